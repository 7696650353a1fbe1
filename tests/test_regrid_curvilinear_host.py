"""Bilinear regridding from curvilinear / rotated source grids (regrid_lat_lon's xESMF branch, reference functions.py:797-810),
the parts that need no GPU: the C-ABI declarations, the settings, the bucket builder of the locate kernel, the `periodic_lon`
rule on 2-D longitudes, the dims check - and the NUMPY STATEMENT OF THE DEFINITION (`locate_statement`, `apply_statement`),
which tries every cell by brute force in the operation order pgw4era5_amd/csrc/pgw_kernels.h documents above k_cell_locate.
tests/test_regrid_curvilinear_hip.py compares the kernels with it bit for bit; here it is checked against ground truth by
construction (a target built from a known cell and known (s, t))."""
import os

import numpy as np
import pytest

from pgw4era5_amd import _lib, functions as F, ncio, settings, synthetic

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = np.finfo(np.float64).eps
STEP_TOL, ACCEPT_TOL, NEWTON_MAX = 1e-14, 1e-10, 20


# ----------------------------------------------------------------------------------------------- the numpy statement
def det3(a, b, c):
    return ((a[..., 0] * (b[..., 1] * c[..., 2] - b[..., 2] * c[..., 1]))
            - (a[..., 1] * (b[..., 0] * c[..., 2] - b[..., 2] * c[..., 0]))) + (a[..., 2] * (b[..., 0] * c[..., 1] - b[..., 1] * c[..., 0]))


def solve_quads(A, B, Cc, D, P):
    """Newton on p(s,t) - r P = 0 for every (target, cell) pair; arrays broadcast to (nt, nc, 3).
    Returns accept (nt, nc) and weights (nt, nc, 4) in corner order A, B, C, D."""
    ab, ad, E, c3 = B - A, D - A, ((A - B) + Cc) - D, -P
    shape = np.broadcast(A, P).shape[:-1]
    s, t, r = np.full(shape, 0.5), np.full(shape, 0.5), np.ones(shape)
    live, conv = np.ones(shape, bool), np.zeros(shape, bool)
    with np.errstate(all='ignore'):
        for _ in range(NEWTON_MAX):
            Fv = (((A + s[..., None] * ab) + t[..., None] * ad) + (s * t)[..., None] * E) - r[..., None] * P
            c1, c2 = ab + t[..., None] * E, ad + s[..., None] * E
            det = det3(c1, c2, c3)
            good = live & ~((det == 0.0) | ~np.isfinite(det))
            ds, dt, dr = det3(Fv, c2, c3) / det, det3(c1, Fv, c3) / det, det3(c1, c2, Fv) / det
            s, t, r = np.where(good, s - ds, s), np.where(good, t - dt, t), np.where(good, r - dr, r)
            good &= np.isfinite(s) & np.isfinite(t) & np.isfinite(r)
            done = good & (np.abs(ds) <= STEP_TOL) & (np.abs(dt) <= STEP_TOL)
            conv |= done
            live = good & ~done
        acc = conv & (r > 0.0) & (s >= -ACCEPT_TOL) & (s <= 1.0 + ACCEPT_TOL) & (t >= -ACCEPT_TOL) & (t <= 1.0 + ACCEPT_TOL)
        s = np.where(s < 0.0, 0.0, np.where(s > 1.0, 1.0, s))
        t = np.where(t < 0.0, 0.0, np.where(t > 1.0, 1.0, t))
        os_, ot = 1.0 - s, 1.0 - t
        w = np.stack([os_ * ot, s * ot, s * t, os_ * t], axis=-1)
    return acc, w


def solve_tris(N, X1, X2, P):
    e1, e2, c3, rhs = X1 - N, X2 - N, -P, -N
    with np.errstate(all='ignore'):
        det = det3(e1, e2, c3)
        u, v, r = det3(rhs, e2, c3) / det, det3(e1, rhs, c3) / det, det3(e1, e2, rhs) / det
        acc = ~((det == 0.0) | ~np.isfinite(det)) & np.isfinite(u) & np.isfinite(v) & np.isfinite(r)
        acc &= (u >= -ACCEPT_TOL) & (v >= -ACCEPT_TOL) & (u + v <= 1.0 + ACCEPT_TOL) & (r > 0.0)
        u = np.where(u < 0.0, 0.0, np.where(u > 1.0, 1.0, u))
        vmax = 1.0 - u
        v = np.where(v < 0.0, 0.0, np.where(v > vmax, vmax, v))
        w = np.stack([(1.0 - u) - v, u, v, np.zeros_like(u)], axis=-1)
    return acc, w


def cell_nodes(ny, nx, periodic):
    """Source-node indices (ncell, 4) of every cell in cell-number order; -1 = absent entry; ny*nx, ny*nx + 1 = the poles."""
    ncx = nx if periodic else nx - 1
    j, i = np.divmod(np.arange((ny - 1) * ncx), ncx)
    ip = (i + 1) % nx
    out = [np.stack([j * nx + i, j * nx + ip, (j + 1) * nx + ip, (j + 1) * nx + i], axis=1)]
    if periodic:
        i = np.arange(nx)
        ip = (i + 1) % nx
        for which, row in ((0, 0), (1, (ny - 1) * nx)):
            out.append(np.stack([np.full(nx, ny * nx + which), row + i, row + ip, np.full(nx, -1)], axis=1))
    return np.concatenate(out, axis=0)


def all_nodes(X, periodic):
    ny = X.shape[0]
    nodes = X.reshape(-1, 3)
    if periodic:
        nodes = np.concatenate([nodes, F.pole_vector(X[0])[None], F.pole_vector(X[ny - 1])[None]], axis=0)
    return nodes


def locate_statement(X, P, periodic):
    """The definition by brute force: every target against every cell, the lowest accepting cell number wins.
    X (ny, nx, 3), P (nt, 3).  Returns idx (nt, 4) int32, w (nt, 4) float64, n_unmapped, cell (nt,) (-1 = unmapped)."""
    ny, nx = X.shape[:2]
    cn = cell_nodes(ny, nx, periodic)
    nodes = all_nodes(X, periodic)
    nq = (ny - 1) * (nx if periodic else nx - 1)
    Pb = P[:, None, :]
    q = cn[:nq]
    acc, w = solve_quads(nodes[q[:, 0]][None], nodes[q[:, 1]][None], nodes[q[:, 2]][None], nodes[q[:, 3]][None], Pb)
    if periodic:
        t = cn[nq:]
        acc_t, w_t = solve_tris(nodes[t[:, 0]][None], nodes[t[:, 1]][None], nodes[t[:, 2]][None], Pb)
        acc, w = np.concatenate([acc, acc_t], axis=1), np.concatenate([w, w_t], axis=1)
    found = acc.any(axis=1)
    cell = np.where(found, acc.argmax(axis=1), -1)
    idx = np.where(found[:, None], cn[np.maximum(cell, 0)], -1).astype(np.int32)
    wt = np.where(found[:, None], w[np.arange(len(P)), np.maximum(cell, 0)], 0.0)
    return idx, wt, int((~found).sum()), cell


def pole_means(src):
    """(nfield, 2): (sum_i v[je, i]) / nx of rows 0 and ny - 1 in index order, float64, NaN propagating."""
    v = src.astype(np.float64)
    return np.stack([np.add.accumulate(v[:, je, :], axis=1)[:, -1] / v.shape[2] for je in (0, v.shape[1] - 1)], axis=1)


def apply_statement(src, idx, w, unmapped_nan=False):
    """src (nfield, ny, nx) float32 / float64 -> (nfield, nt) in src's dtype: acc = w0*v0, then + wk*vk over the present
    entries in order, float64 on the stored values."""
    nf = src.shape[0]
    vals = np.concatenate([src.reshape(nf, -1).astype(np.float64), pole_means(src)], axis=1)
    acc = np.full((nf, len(idx)), np.nan if unmapped_nan else 0.0)
    have = np.zeros(len(idx), bool)
    with np.errstate(all='ignore'):
        for k in range(4):
            present = idx[:, k] >= 0
            term = w[None, :, k] * vals[:, np.maximum(idx[:, k], 0)]
            acc = np.where(present[None], np.where(have[None], acc + term, term), acc)
            have |= present
        return acc.astype(src.dtype)


# ----------------------------------------------------------------------------------------------- grids and targets
def jittered_grid(ny, nx, lat, lon, periodic, seed, jit=0.15):
    """Unit vectors (ny, nx, 3) of a grid regular in (lat, lon) over the given ranges, every node moved by up to `jit` of
    the spacing: logically rectangular, convex cells, 2-D coordinates."""
    rng = np.random.default_rng(seed)
    la = np.linspace(lat[0], lat[1], ny)
    lo = lon[0] + (lon[1] - lon[0]) * np.arange(nx) / (nx if periodic else nx - 1)
    la2 = la[:, None] + jit * (la[1] - la[0]) * rng.uniform(-1, 1, (ny, nx))
    lo2 = lo[None, :] + jit * (lo[1] - lo[0]) * rng.uniform(-1, 1, (ny, nx))
    return F.unit_vectors(la2, lo2)


def rotated_grid():
    _, _, lat, lon = synthetic.rotated_pole_grid(24, 48)
    return F.unit_vectors(lat, lon)


GRIDS = {
    '2x2': lambda: (jittered_grid(2, 2, (10, 30), (5, 30), False, 1), False),
    '3x4': lambda: (jittered_grid(3, 4, (-20, 25), (100, 160), False, 2), False),
    '5x7': lambda: (jittered_grid(5, 7, (35, 60), (-10, 40), False, 3), False),
    '5x7p': lambda: (jittered_grid(5, 7, (-60, 60), (0, 360), True, 4, jit=0.08), True),
    '5x12p_30deg': lambda: (jittered_grid(5, 12, (-60, 60), (0, 360), True, 5, jit=0.05), True),
    'rot24x48': lambda: (rotated_grid(), False),
}


def normalise(v):
    return v / np.sqrt((v[..., 0] * v[..., 0] + v[..., 1] * v[..., 1]) + v[..., 2] * v[..., 2])[..., None]


def truth_targets(X, periodic, n, seed):
    """n targets with a known answer: cell c and (s, t) in [0.05, 0.95]^2, P = normalise(p(s, t)); cap triangles with
    (u, v), u, v >= 0.05, u + v <= 0.95.  Returns P (n, 3), cell (n,), st (n, 2)."""
    rng = np.random.default_rng(seed)
    ny, nx = X.shape[:2]
    cn = cell_nodes(ny, nx, periodic)
    nodes = all_nodes(X, periodic)
    cell = rng.integers(0, len(cn), n)
    if n >= len(cn):
        cell[:len(cn)] = np.arange(len(cn))                      # every cell at least once when there is room
    a, b = rng.uniform(0, 1, n), rng.uniform(0, 1, n)
    tri = cn[cell, 3] < 0
    flip = tri & (a + b > 1)
    a, b = np.where(flip, 1 - a, a), np.where(flip, 1 - b, b)
    s = np.where(tri, 0.05 + 0.85 * a, 0.05 + 0.9 * a)
    t = np.where(tri, 0.05 + 0.85 * b, 0.05 + 0.9 * b)
    A, B, Cc = nodes[cn[cell, 0]], nodes[cn[cell, 1]], nodes[cn[cell, 2]]
    D = nodes[np.maximum(cn[cell, 3], 0)]
    pq = A + s[:, None] * (B - A) + t[:, None] * (D - A) + (s * t)[:, None] * (A - B + Cc - D)
    pt = A + s[:, None] * (B - A) + t[:, None] * (Cc - A)
    return normalise(np.where(tri[:, None], pt, pq)), cell, np.stack([s, t], axis=1)


def shortest_chord(X, periodic):
    ny, nx = X.shape[:2]
    cn = cell_nodes(ny, nx, periodic)
    nodes = all_nodes(X, periodic)
    best = np.inf
    for a, b in ((0, 1), (1, 2), (2, 3), (3, 0), (0, 2)):
        ok = (cn[:, a] >= 0) & (cn[:, b] >= 0)
        d = nodes[cn[ok, a]] - nodes[cn[ok, b]]
        d = np.sqrt((d ** 2).sum(axis=1))
        best = min(best, d[d > 0].min())
    return best


def recovered_st(idx, w):
    """(s, t) of a quad entry = (wB + wC, wC + wD); (u, v) of a triangle entry = (w1, w2)."""
    tri = idx[:, 3] < 0
    return np.stack([np.where(tri, w[:, 1], w[:, 1] + w[:, 2]), np.where(tri, w[:, 2], w[:, 2] + w[:, 3])], axis=1)


def check_truth(X, periodic, idx, w, cell, st):
    """Ground truth by construction: the cell's four indices, no exceptions, and (s, t) within 64 eps / (shortest chord of
    the grid's cells) - eps times the conditioning of the solve, with margin."""
    cn = cell_nodes(X.shape[0], X.shape[1], periodic)
    np.testing.assert_array_equal(idx, cn[cell])
    tol = 64 * EPS / shortest_chord(X, periodic)
    err = np.abs(recovered_st(idx, w) - st).max()
    print('max |(s,t) - truth| = %.3e (tolerance %.3e)' % (err, tol))
    assert err <= tol


# ----------------------------------------------------------------------------------------------- tests
def test_header_and_lib_agree():
    hdr = open(os.path.join(ROOT, 'include', 'pgw_hip.h')).read()
    for name in ('pgw_bilinear_locate', 'pgw_regrid_sparse'):
        assert name in _lib.SIGNATURES and name + '(' in hdr
    assert 'PGW_K_CELL_LOCATE = %d' % _lib.KERNEL_IDS['cell_locate'] in hdr and _lib.KERNEL_IDS['cell_locate'] == 26
    assert 'PGW_K_REGRID_SPARSE = %d' % _lib.KERNEL_IDS['regrid_sparse'] in hdr and _lib.KERNEL_IDS['regrid_sparse'] == 27
    assert 'PGW_K_COUNT = 28' in hdr and len(_lib.KERNEL_IDS) == 28
    assert 'PGW_OPT_SPARSE_DIRECT = %d' % _lib.OPTIONS['sparse_direct'] in hdr
    assert 'PGW_OPT_COUNT = %d' % len(_lib.OPTIONS) in hdr
    assert len(_lib.SIGNATURES['pgw_bilinear_locate'][1]) == 13
    assert len(_lib.SIGNATURES['pgw_regrid_sparse'][1]) == 11
    for cite in ('functions.py:797-810', 'settings.py:117-129'):           # each entry cites the reference lines it replaces
        assert cite in hdr


def test_settings_defaults():
    assert settings.i_use_xesmf_regridding == 0
    assert settings.xesmf_unmapped_to_nan is False


def host_bucket(P, nb):
    c = np.clip(((P + 1.0) * 0.5 * nb).astype(np.int64), 0, nb - 1)
    return (c[:, 0] * nb + c[:, 1]) * nb + c[:, 2]


@pytest.mark.parametrize('name', sorted(GRIDS))
@pytest.mark.parametrize('nb', [None, 7])
def test_bucket_lists_hold_the_true_cell(name, nb):
    X, periodic = GRIDS[name]()
    P, cell, _ = truth_targets(X, periodic, 400, seed=11)
    nb, start, cells = F.curvilinear_buckets(X, periodic, nb)
    assert start[0] == 0 and start[-1] == len(cells) and len(start) == nb ** 3 + 1
    b = host_bucket(P, nb)
    for k in range(len(P)):
        lst = cells[start[b[k]]:start[b[k] + 1]]
        assert cell[k] in lst, (name, k)
        assert (np.diff(lst) > 0).all()                            # ascending: the first accepting candidate is the lowest


def test_bucket_lists_hold_every_accepting_cell_on_edges_and_nodes():
    """Targets on nodes and on shared edges are accepted by several cells (tolerance 1e-10): all of them must be listed."""
    X, periodic = GRIDS['5x7p']()
    nodes = all_nodes(X, periodic)
    mids = normalise(0.5 * (X[:, :-1] + X[:, 1:])).reshape(-1, 3)
    P = np.concatenate([nodes, mids], axis=0)
    cn = cell_nodes(5, 7, periodic)
    nq = 4 * 7
    acc, _ = solve_quads(*(nodes[cn[:nq, k]][None] for k in range(4)), P[:, None, :])
    acc_t, _ = solve_tris(*(nodes[cn[nq:, k]][None] for k in range(3)), P[:, None, :])
    acc = np.concatenate([acc, acc_t], axis=1)
    assert (acc.sum(axis=1) >= 2).all()
    nb, start, cells = F.curvilinear_buckets(X, periodic)
    b = host_bucket(P, nb)
    for k in range(len(P)):
        assert set(np.nonzero(acc[k])[0]) <= set(cells[start[b[k]]:start[b[k] + 1]])


def test_bucket_builder_skips_nan_cells():
    X, periodic = GRIDS['3x4']()
    X = X.copy()
    X[1, 1] = np.nan
    _, _, cells = F.curvilinear_buckets(X, periodic)
    assert set(cells) == {2, 5}                                   # the four cells around node (1, 1) are listed nowhere


@pytest.mark.parametrize('name', sorted(GRIDS))
def test_statement_against_ground_truth(name):
    X, periodic = GRIDS[name]()
    P, cell, st = truth_targets(X, periodic, 65 if name == 'rot24x48' else 257, seed=7)
    idx, w, n_un, got = locate_statement(X, P, periodic)
    assert n_un == 0
    np.testing.assert_array_equal(got, cell)
    check_truth(X, periodic, idx, w, cell, st)


def test_statement_apply_order_and_unmapped():
    """A self-check of the checker: `apply_statement` (what the GPU tests hold k_regrid_sparse to) on a case worked by hand -
    the order of the sum, an absent entry, a pole entry, an unmapped target.  It runs no code of the package."""
    src = np.arange(12, dtype=np.float32).reshape(1, 3, 4)
    idx = np.array([[0, 1, 5, 4], [-1, -1, -1, -1], [12, 0, 1, -1]], dtype=np.int32)
    w = np.array([[0.25, 0.25, 0.25, 0.25], [0, 0, 0, 0], [0.5, 0.25, 0.25, 0]])
    out = apply_statement(src, idx, w)
    np.testing.assert_array_equal(out, np.array([[2.5, 0.0, 0.5 * 1.5 + 0.25]], dtype=np.float32))
    assert np.isnan(apply_statement(src, idx, w, unmapped_nan=True)[0, 1])


def test_periodic_rule_on_2d_longitudes():
    lon = np.arange(48) * 7.5
    lat = np.linspace(-80, 80, 24)
    lat2, lon2 = np.meshgrid(lat, lon, indexing='ij')
    assert F.periodic_lon_rule(lon2) is True and F.periodic_lon_rule(lon) is True
    assert F.periodic_lon_rule(lon2[:, :40]) is False
    _, _, rlat2, rlon2 = synthetic.rotated_pole_grid()
    assert F.periodic_lon_rule(rlon2) is False
    # np.diff along the LAST axis: the same numbers laid out the other way round differ along it by 0, so the rule sees
    # max - min alone
    assert F.periodic_lon_rule(lon2.T.copy()) is False
    assert F.periodic_lon_rule(lon2[:, :47] + np.linspace(0, 1.0, 24)[:, None]) == bool(7.5 + 345.0 + 1.0 >= 359.9)


def test_wrong_dims_raise_value_error():
    ds = synthetic.make_rotated_delta(nrlat=4, nrlon=5, nplev=2, ntime=1)
    ds['swapped'] = ncio.Field(np.zeros((1, 5, 4)), ('time', 'rlon', 'rlat'))
    ds['flat'] = ncio.Field(np.zeros((1, 4)), ('time', 'rlat'))
    era = ncio.Dataset()
    era['lat'] = ncio.Field(np.array([45.0, 46.0]), ('lat',))
    era['lon'] = ncio.Field(np.array([10.0, 11.0, 12.0]), ('lon',))
    for name in ('swapped', 'flat'):
        with pytest.raises(ValueError, match='horizontal dimensions'):
            F.regrid_lat_lon(ds, era, name, i_use_xesmf=1)


def test_synthetic_rotated_delta_is_curvilinear():
    ds = synthetic.make_rotated_delta()
    assert ds['lat'].dims == ds['lon'].dims == ('rlat', 'rlon') and ds['ta'].dims == ('time', 'plev', 'rlat', 'rlon')
    lat, lon = ds['lat'].values, ds['lon'].values
    assert np.ptp(lat[0]) > 1.0 and np.ptp(lon[:, 0]) > 1.0        # rows are not parallels, columns not meridians
    X = F.unit_vectors(lat, lon)
    np.testing.assert_allclose((X ** 2).sum(axis=-1), 1.0, rtol=0, atol=4 * EPS)
