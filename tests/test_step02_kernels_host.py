"""Plain-numpy references of the two step_02 kernels, and the host tests that keep them honest.

`gauss_reference` and `harmonic_reference` restate the definitions written above k_gauss_interp and k_harmonic_smooth in
pgw4era5_amd/csrc/pgw_kernels.h.  Every decision the kernels take on a float64 value (inside the radius, coincident
point, underflow of a weight to 0) is taken here on the same float64 value, formed by the same operations in the same
order; every sum and product whose rounding is the kernel's own error is carried in np.longdouble.  The GPU tests of
tests/test_step02_kernels_hip.py import the references from here.  No GPU is needed in this file."""
import numpy as np

from oracle import pgw_oracle as O

EPS = float(np.finfo(np.float64).eps)
HIT_TOL = 256.0 * EPS                                  # vtkMathUtilities::FuzzyCompare(d2, 0.0, eps * 256)
LD = np.longdouble


# ------------------------------------------------------------------ the references
def gauss_geometry(x, y, sx, sy, radius, sharpness):
    """One target against the whole cloud, in float64 as the kernel forms it: indices of the points with d2 <= r2 (input
    order), which of them are coincident (d2 < 256 eps), and their weights exp(-f2 d2)."""
    r2 = radius * radius
    f2 = (sharpness * sharpness) / (radius * radius)
    dx, dy = x - sx, y - sy
    d2 = dx * dx + dy * dy                              # two products and one sum, each rounded (no contraction)
    idx = np.flatnonzero(d2 <= r2)
    with np.errstate(under='ignore'):
        w = np.exp(-f2 * d2[idx])
    return idx, d2[idx] < HIT_TOL, w


def gauss_exact_hits(tx, ty, sx, sy, sval, radius):
    """[nm, ntarg] bool: the months in which a target takes the exact-hit branch (a coincident point valid in that month)."""
    tx, ty, sx, sy = (np.asarray(a, dtype=np.float64).reshape(-1) for a in (tx, ty, sx, sy))
    sval = np.asarray(sval, dtype=np.float64).reshape(len(sx), -1)
    hits = np.zeros((sval.shape[1], len(tx)), dtype=bool)
    for i in range(len(tx)):
        if np.isnan(tx[i]) or np.isnan(ty[i]):
            continue
        idx, exact, _ = gauss_geometry(tx[i], ty[i], sx, sy, radius, 1.0)
        hits[:, i] = (exact[:, None] & ~np.isnan(sval[idx])).any(axis=0)
    return hits


def gauss_reference(tx, ty, sx, sy, sval, radius, sharpness):
    """Brute force over all pairs.  sval [nsrc, nm].  Returns (out [nm, ntarg] longdouble, n_acc [nm, ntarg] int,
    scale [nm, ntarg] longdouble): the interpolated value, the number of accepted points (inside the radius, valid in
    that month) and sum w |v| / sum w.  A month's NaN values are skipped; a coincident valid point gives its value (the
    first in input order); no accepted point, sum w == 0 or a NaN target coordinate give NaN."""
    tx, ty, sx, sy = (np.asarray(a, dtype=np.float64).reshape(-1) for a in (tx, ty, sx, sy))
    sval = np.asarray(sval, dtype=np.float64).reshape(len(sx), -1)
    nm, ntarg = sval.shape[1], len(tx)
    out = np.full((nm, ntarg), np.nan, dtype=LD)
    scale = np.full((nm, ntarg), np.nan, dtype=LD)
    n_acc = np.zeros((nm, ntarg), dtype=np.int64)
    for i in range(ntarg):
        if np.isnan(tx[i]) or np.isnan(ty[i]):
            continue
        idx, exact, w = gauss_geometry(tx[i], ty[i], sx, sy, radius, sharpness)
        if not len(idx):
            continue
        v = sval[idx]
        ok = ~np.isnan(v)
        wl = np.where(ok, w[:, None], 0.0).astype(LD)                       # [nacc, nm]
        vl = np.where(ok, v, 0.0).astype(LD)
        sw = wl.sum(axis=0)
        n_acc[:, i] = ok.sum(axis=0)
        pos = sw > 0
        den = np.where(pos, sw, LD(1))
        out[:, i] = np.where(pos, (wl * vl).sum(axis=0) / den, LD(np.nan))
        scale[:, i] = np.where(pos, (wl * np.abs(vl)).sum(axis=0) / den, LD(np.nan))
        for m in range(nm):
            hit = np.flatnonzero(exact & ok[:, m])
            if len(hit):
                out[m, i] = v[hit[0], m]
    return out, n_acc, scale


def harmonic_reference(x):
    """x [ntime, inner] (float32 or float64, widened exactly) -> longdouble [ntime, inner]: mean + the first three
    harmonics with the tables the kernel gets (functions.harmonic_tables).  A column holding a NaN comes back all NaN."""
    from pgw4era5_amd import functions as F
    x = np.asarray(x)
    nt = x.shape[0]
    xl = x.reshape(nt, -1).astype(LD)
    cos_t, sin_t = F.harmonic_tables(nt)
    res = np.broadcast_to(xl.sum(axis=0) / LD(nt), xl.shape).copy()
    for k in range(3):
        c, s = cos_t[k].astype(LD)[:, None], sin_t[k].astype(LD)[:, None]
        a = LD(2) * (xl * c).sum(axis=0) / LD(nt)
        b = LD(2) * (xl * s).sum(axis=0) / LD(nt)
        res += a[None, :] * c + b[None, :] * s
    res[:, np.isnan(xl).any(axis=0)] = np.nan
    return res.reshape(x.shape)


# ------------------------------------------------------------------ host tests of the references
def test_longdouble_is_wider_than_float64():
    """The references are only a yardstick for fp64 kernels where longdouble carries more bits."""
    assert np.finfo(LD).eps <= EPS / 1024


def _planar_cloud(seed, nsrc=300):
    rng = np.random.default_rng(seed)
    sx, sy = rng.uniform(0.0, 6.0, nsrc), rng.uniform(0.0, 6.0, nsrc)
    val = rng.normal(250.0, 20.0, nsrc)
    return rng, sx, sy, val


def test_gauss_reference_agrees_with_the_oracle_loop(monkeypatch):
    """Against the inner loop of O.nan_ignoring_interp (normalise the weights, then sum, all float64) on a planar cloud:
    the oracle's geodesy is replaced by the identity, its two shifted copies of the cloud lie far outside every radius."""
    rng, sx, sy, val = _planar_cloud(11)
    val[rng.choice(len(val), 25, replace=False)] = np.nan                  # removed from the cloud by the oracle
    ex, ey = np.linspace(-0.5, 6.5, 13), np.linspace(-0.75, 6.25, 12)
    sx[0], sy[0] = ex[4], ey[7]                                            # a coincident target
    sx[1], sy[1] = ex[9], ey[2]                                            # a coincident target whose point is NaN
    val[0], val[1] = 263.0, np.nan
    monkeypatch.setattr(O, 'planar_metres', lambda lat, lon: (np.asarray(lat, dtype=np.float64),
                                                              np.asarray(lon, dtype=np.float64),
                                                              np.full(len(lat), 1.0e3)))
    radius, sharp = 1.0, 4.0
    want = O.nan_ignoring_interp(np.zeros((len(ex), len(ey))), ex, ey, sx, sy, val, radius, sharp)
    tx, ty = np.repeat(ex, len(ey)), np.tile(ey, len(ex))
    got, n_acc, scale = gauss_reference(tx, ty, sx, sy, val[:, None], radius, sharp)
    got, want = got[0], want.reshape(-1)
    assert 0 < np.isnan(want).sum() < len(want) // 4                       # the corners of the target grid see no point
    np.testing.assert_array_equal(np.isnan(got), np.isnan(want))
    np.testing.assert_array_equal(n_acc[0] == 0, np.isnan(want))
    ok = ~np.isnan(want)
    err = np.abs(got[ok] - want[ok].astype(LD)) / np.abs(want[ok])
    assert err.max() <= 1e-13, err.max()
    assert got[4 * len(ey) + 7] == 263.0                                   # the hit, exactly
    hits = gauss_exact_hits(tx, ty, sx, sy, val[:, None], radius)
    assert hits.sum() == 1 and hits[0, 4 * len(ey) + 7]
    ok &= ~hits[0]                                                         # (a hit's scale is that of the weighted mean)
    assert (scale[0][ok] >= np.abs(got[ok]) * (1 - 1e-15)).all()


def test_gauss_reference_constant_hit_order_and_nan_months():
    rng, sx, sy, _ = _planar_cloud(12, nsrc=200)
    tx, ty = rng.uniform(0.5, 5.5, 40), rng.uniform(0.5, 5.5, 40)
    # a constant field comes back as the constant wherever a point is in reach
    out, n_acc, scale = gauss_reference(tx, ty, sx, sy, np.full((200, 2), -3.25), 1.0, 4.0)
    assert (n_acc > 0).all() and (np.abs(out + LD(3.25)) <= 1e-16 * 3.25).all() and (np.abs(scale - LD(3.25)) <= 1e-16 * 3.25).all()
    # coincident points: the value of the first valid one in input order, per month; other months are weighted means
    val = rng.normal(0.0, 5.0, (200, 3))
    sx[7], sy[7] = sx[3], sy[3]                                            # point 7 coincides with point 3
    val[3, 1] = np.nan
    tx[0], ty[0] = sx[3], sy[3]
    tx[1], ty[1] = np.nan, 2.0
    tx[2], ty[2] = 40.0, 40.0                                              # nothing in reach
    out, n_acc, scale = gauss_reference(tx, ty, sx, sy, val, 1.0, 4.0)
    assert out[0, 0] == val[3, 0] and out[2, 0] == val[3, 2] and out[1, 0] == val[7, 1]
    assert n_acc[1, 0] == n_acc[0, 0] - 1
    assert np.isnan(out[:, 1]).all() and (n_acc[:, 1] == 0).all()
    assert np.isnan(out[:, 2]).all() and (n_acc[:, 2] == 0).all() and np.isnan(scale[:, 2]).all()
    hits = gauss_exact_hits(tx, ty, sx, sy, val, 1.0)
    assert hits[:, 0].all() and not hits[:, 1:].any()
    # a NaN month changes that month only, and there it is the mean over the remaining points
    val2 = val.copy()
    val2[:, 1] = np.where(rng.uniform(size=200) < 0.3, np.nan, val[:, 1])
    out2, n2, _ = gauss_reference(tx, ty, sx, sy, val2, 1.0, 4.0)
    for m in (0, 2):
        np.testing.assert_array_equal(out2[m], out[m])
    keep = ~np.isnan(val2[:, 1])
    out3, n3, _ = gauss_reference(tx, ty, sx[keep], sy[keep], val2[keep, 1:2], 1.0, 4.0)
    np.testing.assert_array_equal(n2[1], n3[0])
    np.testing.assert_array_equal(np.isnan(out2[1]), np.isnan(out3[0]))
    seen = ~np.isnan(out3[0])                                              # (the same longdouble sums, paired differently)
    assert seen.sum() > 30 and np.abs(out2[1][seen] - out3[0][seen]).max() <= 1e-17 * np.nanmax(np.abs(val))
    # weights that underflow to 0 in float64: no value
    out4, n4, _ = gauss_reference(np.array([0.0]), np.array([0.0]), np.array([0.95]), np.array([0.0]), np.array([[1.0]]), 1.0, 30.0)
    assert n4[0, 0] == 1 and np.isnan(out4[0, 0])


def test_harmonic_reference_agrees_with_the_oracle():
    rng = np.random.default_rng(13)
    for shape in [(365, 3, 5), (366, 2, 2, 3), (8, 1, 4), (17, 2, 3)]:
        x = rng.normal(250.0, 20.0, shape)
        x[shape[0] // 2, ..., 1] = np.nan
        want = O.filter_data_array(x)
        got = harmonic_reference(x.reshape(shape[0], -1)).reshape(shape)
        np.testing.assert_array_equal(np.isnan(got), np.isnan(want))
        assert np.isnan(want[:, ..., 1]).all() and not np.isnan(want[:, ..., 0]).any()
        ok = ~np.isnan(want)
        assert np.abs(got[ok] - want[ok].astype(LD)).max() <= 1e-12 * np.abs(x[ok]).max()
    x32 = rng.normal(250.0, 20.0, (24, 7)).astype(np.float32)
    np.testing.assert_array_equal(harmonic_reference(x32), harmonic_reference(x32.astype(np.float64)))


def harmonic_series(ntime, inner, seed):
    """Columns that are exactly mean + three harmonics of the kernel's tables (up to the rounding of each value to float64)."""
    from pgw4era5_amd import functions as F
    rng = np.random.default_rng(seed)
    cos_t, sin_t = (t.astype(LD) for t in F.harmonic_tables(ntime))
    x = np.broadcast_to(rng.normal(250.0, 20.0, inner).astype(LD), (ntime, inner)).copy()
    for k in range(3):
        x += rng.normal(0.0, 20.0 / (k + 1), inner).astype(LD)[None, :] * cos_t[k][:, None]
        x += rng.normal(0.0, 20.0 / (k + 1), inner).astype(LD)[None, :] * sin_t[k][:, None]
    return x.astype(np.float64)


def test_harmonic_reference_reproduces_a_harmonic_series():
    """To 1e-13 of the series' scale: the table entries are cos / sin of a rounded argument (up to 6 pi, so off by up to
    2e-15), which makes the seven basis vectors orthogonal to about that much and no better."""
    for ntime in (8, 9, 17, 365, 366):
        x = harmonic_series(ntime, 5, ntime)
        assert np.abs(harmonic_reference(x) - x.astype(LD)).max() <= 1e-13 * np.abs(x).max()


def test_planar_metres_host_keeps_nan_points_to_themselves():
    """geodesy.planar_metres: a NaN latitude or longitude gives NaN in lon_m (and in lat_m for a NaN latitude); every other
    point is the bits of a run without the NaN points."""
    from pgw4era5_amd import geodesy as G
    rng = np.random.default_rng(14)
    lat, lon = rng.uniform(-89.0, 89.0, 300), rng.uniform(-179.0, 179.0, 300)
    clean = G.planar_metres(lat, lon)
    lat2, lon2 = lat.copy(), lon.copy()
    nan_lat, nan_lon, nan_both = [5, 64, 299], [0, 63, 130], [17]
    lat2[nan_lat + nan_both] = np.nan
    lon2[nan_lon + nan_both] = np.nan
    got = G.planar_metres(lat2, lon2)
    assert np.isnan(got[1][nan_lat + nan_lon + nan_both]).all() and np.isnan(got[0][nan_lat + nan_both]).all()
    other = np.ones(300, dtype=bool)
    other[nan_lat + nan_lon + nan_both] = False
    for g, c in zip(got, clean):
        np.testing.assert_array_equal(g[other].view(np.uint64), c[other].view(np.uint64))
    np.testing.assert_array_equal(got[0][nan_lon].view(np.uint64), clean[0][nan_lon].view(np.uint64))   # lat_m of a NaN longitude
