"""The step_02 kernels at their edges: `pgw_gauss_interp`, `pgw_harmonic_smooth` and `pgw_planar_metres` called directly
through the C API, and the host branches of `functions.gauss_interp_fields`.

The references are the longdouble brute-force restatements of tests/test_step02_kernels_host.py.  The tolerances are
derived, evaluated per target / per column from the reference's own outputs:

  gauss     where the reference takes the exact-hit branch or returns NaN: equality (of the bits / of the NaN mask);
            elsewhere |got - ref| <= (n_acc + 40) eps scale, n_acc accepted points and scale = sum w |v| / sum w: the two
            sequential sums of n_acc terms, the device exp against numpy's (an ulp, on an argument of at most 16 in size),
            the division and slack.
  harmonic  float64: |got - ref| <= 13 (ntime + 4) eps max|x| of the column - seven sequential sums of ntime terms with
            |cos|, |sin| <= 1, each entering the result with a factor of at most 2, plus the final adds; float32: the same
            plus 2^-24 |ref| for the one rounding of the result to float32.

Each case asserts its own intended condition (run lengths read from `cell_start`, the number of accepted points at the
radius edge, which targets lie outside the cell grid, ...), so that a change to a helper cannot turn an edge case into an
ordinary one unnoticed.  The largest observed error of each kernel as a fraction of its bound is printed at the end of
the module (run with -s)."""
import ctypes as C

import numpy as np
import pytest

import test_step02_kernels_host as H
from test_step02_kernels_host import EPS, HIT_TOL, LD

pytestmark = pytest.mark.gpu

BLOCK = 256                       # threads (= targets / columns) per block of both kernels
CHUNK = 256                       # GAUSS_CHUNK: source points staged per pass through LDS
_dp = C.POINTER(C.c_double)
SENTINEL = -777.0                 # what the output buffers hold before a call: every element must be overwritten
WORST = {}                        # kernel -> largest observed error / bound


@pytest.fixture(scope='module')
def ctx():
    from pgw4era5_amd.device import default_context
    yield default_context()
    if WORST:
        print('\nlargest observed error as a fraction of the derived bound: ' +
              ', '.join('%s %.3f' % kv for kv in sorted(WORST.items())))


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype == np.float64 else np.uint32)


def _assert_same_bits(a, b, msg=''):
    assert a.dtype == b.dtype and a.shape == b.shape, msg
    np.testing.assert_array_equal(_bits(a), _bits(b), err_msg=msg)


def _record(name, err, bound):
    pos = bound > 0
    if pos.any():
        WORST[name] = max(WORST.get(name, 0.0), float((err[pos] / bound[pos]).max()))


# ------------------------------------------------------------------ pgw_gauss_interp
class Cloud:
    """Source points binned into ncx x ncy square cells of edge h from (x0, y0) and sorted by cell, with the numpy lines
    of functions.gauss_interp_fields; `sx`, `sy`, `sv` are the sorted arrays, i.e. the order handed to the kernel."""

    def __init__(self, sx, sy, sv, ncx=6, ncy=6, x0=0.0, y0=0.0, h=1.0):
        sx, sy = np.asarray(sx, dtype=np.float64), np.asarray(sy, dtype=np.float64)
        sv = np.asarray(sv, dtype=np.float64)
        sv = sv.reshape(len(sx), -1 if len(sx) else sv.shape[-1])
        ix, iy = ((sx - x0) // h).astype(np.int64), ((sy - y0) // h).astype(np.int64)
        assert ((ix >= 0) & (ix < ncx) & (iy >= 0) & (iy < ncy)).all(), 'source point outside the cell grid'
        cid = ix * ncy + iy
        order = np.argsort(cid, kind='stable')
        self.sx, self.sy, self.sv, cid = sx[order], sy[order], np.ascontiguousarray(sv[order]), cid[order]
        self.cell_start = np.searchsorted(cid, np.arange(ncx * ncy + 1)).astype(np.int32)
        assert self.cell_start[0] == 0 and self.cell_start[-1] == len(sx) and (np.diff(self.cell_start) >= 0).all()
        self.order, self.ncx, self.ncy, self.x0, self.y0, self.h = order, ncx, ncy, x0, y0, h

    def count(self, cx, cy):
        return int(self.cell_start[cx * self.ncy + cy + 1] - self.cell_start[cx * self.ncy + cy])

    def target_cells(self, tx, ty):
        """The kernel's cell indices of the targets (floor((x - x0) * (1 / h)))."""
        inv_h = 1.0 / self.h
        return np.floor((tx - self.x0) * inv_h), np.floor((ty - self.y0) * inv_h)

    def block_runs(self, tx, ty, boxes=False):
        """Per block of 256 targets: {ix: number of points the block stages for cell row ix}, from the box of the block's
        active targets, its clamps and `cell_start` - as the kernel forms them.  None for a block with no active target.
        boxes=True: the clamped boxes (ix_lo, ix_hi, iy_lo, iy_hi) instead."""
        res = []
        for b in range(0, len(tx), BLOCK):
            x, y = tx[b:b + BLOCK], ty[b:b + BLOCK]
            act = ~(np.isnan(x) | np.isnan(y))
            if not act.any():
                res.append(None)
                continue
            cx, cy = self.target_cells(x[act], y[act])
            ix_lo, ix_hi = max(int(cx.min()) - 1, 0), min(int(cx.max()) + 1, self.ncx - 1)
            iy_lo, iy_hi = max(int(cy.min()) - 1, 0), min(int(cy.max()) + 1, self.ncy - 1)
            if boxes:
                res.append((ix_lo, ix_hi, iy_lo, iy_hi))
                continue
            runs = {}
            if iy_lo <= iy_hi:
                for ix in range(ix_lo, ix_hi + 1):
                    runs[ix] = int(self.cell_start[ix * self.ncy + iy_hi + 1] - self.cell_start[ix * self.ncy + iy_lo])
            res.append(runs)
        return res


def _gauss(ctx, cloud, tx, ty, sv=None, radius=1.0, sharpness=4.0, nfield=None, cell=None, null_sources=False):
    """One pgw_gauss_interp call: out [nm, ntarg]."""
    sv = cloud.sv if sv is None else np.ascontiguousarray(sv, dtype=np.float64)
    nm = sv.shape[1] if nfield is None else nfield
    tx, ty = np.ascontiguousarray(tx, dtype=np.float64), np.ascontiguousarray(ty, dtype=np.float64)
    ntarg, nsrc = len(tx), len(cloud.sx)
    assert sv.shape[0] == nsrc and len(ty) == ntarg
    d_tx, d_ty = ctx.to_device(tx), ctx.to_device(ty)
    d_cs = ctx.empty(cloud.cell_start.shape, np.int32).copy_from(cloud.cell_start)
    if null_sources:
        assert nsrc == 0
        p_sx = p_sy = p_sv = None
    else:                                                 # an empty cloud: one unused element, as gauss_interp_fields uploads
        d_sx, d_sy = ctx.to_device(cloud.sx if nsrc else np.zeros(1)), ctx.to_device(cloud.sy if nsrc else np.zeros(1))
        d_sv = ctx.to_device(sv if nsrc else np.zeros((1, max(nm, 1))))
        p_sx, p_sy, p_sv = d_sx.ptr, d_sy.ptr, d_sv.ptr
    d_out = ctx.to_device(np.full((max(nm, 1), ntarg), SENTINEL))
    ctx._check(ctx.lib.pgw_gauss_interp(ctx.handle, ntarg, d_tx.ptr, d_ty.ptr, cloud.ncx, cloud.ncy, cloud.x0, cloud.y0,
                                        cloud.h if cell is None else cell, d_cs.ptr, nsrc, p_sx, p_sy, p_sv, nm,
                                        float(radius), float(sharpness), d_out.ptr))
    return d_out.numpy()


def _check_gauss(got, cloud, tx, ty, sv=None, radius=1.0, sharpness=4.0):
    """got [nm, ntarg] against gauss_reference on the arrays in the order handed to the kernel.  Returns (ref, n_acc, hits)."""
    sv = cloud.sv if sv is None else sv
    ref, n_acc, scale = H.gauss_reference(tx, ty, cloud.sx, cloud.sy, sv, radius, sharpness)
    hits = H.gauss_exact_hits(tx, ty, cloud.sx, cloud.sy, sv, radius)
    assert got.shape == ref.shape and got.dtype == np.float64
    nan = np.isnan(ref)
    np.testing.assert_array_equal(np.isnan(got), nan, err_msg='NaN mask')
    _assert_same_bits(got[hits], ref[hits].astype(np.float64), 'exact hits')
    rest = ~nan & ~hits
    err = np.abs(got[rest].astype(LD) - ref[rest])
    bound = (n_acc[rest] + 40) * LD(EPS) * scale[rest]
    bad = np.flatnonzero(err > bound)
    if bad.size:
        m, i = (a[bad[:5]] for a in np.nonzero(rest))
        raise AssertionError('%d of %d values beyond (n_acc + 40) eps scale; worst %.2f of the bound; month %s target %s got %s ref %s n_acc %s'
                             % (bad.size, err.size, float((err[bad] / bound[bad]).max()), m, i, got[rest][bad[:5]],
                                ref[rest][bad[:5]].astype(np.float64), n_acc[rest][bad[:5]]))
    _record('k_gauss_interp', err, bound)
    return ref, n_acc, hits


def _background(rng, per_cell, nm, ncx=6, ncy=6, nan_fraction=0.0):
    """`per_cell` points in every unit cell of the grid, values of both signs."""
    cx, cy = np.meshgrid(np.arange(ncx), np.arange(ncy), indexing='ij')
    sx = (np.repeat(cx.ravel(), per_cell) + rng.uniform(0.0, 1.0, ncx * ncy * per_cell))
    sy = (np.repeat(cy.ravel(), per_cell) + rng.uniform(0.0, 1.0, ncx * ncy * per_cell))
    sv = rng.normal(0.0, 5.0, (len(sx), nm))
    if nan_fraction:
        sv[rng.uniform(size=sv.shape) < nan_fraction] = np.nan
    p = rng.permutation(len(sx))                          # not cell-sorted: the sort of Cloud has something to do
    return sx[p], sy[p], sv[p]


def _packed_cloud(rng, run, nm):
    """Three points in every cell plus as many in cell (3, 3) as make the run of cell row 3 over the cells 1 .. 5 `run` long."""
    bx, by, bv = _background(rng, 3, nm)
    npack = run - 5 * 3
    sx = np.concatenate([bx, 3.0 + rng.uniform(0.0, 1.0, npack)])
    sy = np.concatenate([by, 3.0 + rng.uniform(0.0, 1.0, npack)])
    return Cloud(sx, sy, np.concatenate([bv, rng.normal(0.0, 5.0, (npack, nm))]))


def _targets_around_cell_33(rng, n):
    tx, ty = rng.uniform(2.0, 5.0, n), rng.uniform(2.0, 5.0, n)
    tx[:4], ty[:4] = [2.1, 4.9, 2.2, 4.8], [2.3, 4.7, 4.9, 2.05]          # the box is the cells 2 .. 4 both ways
    return tx, ty


@pytest.mark.parametrize('run', [255, 256, 257, 512, 513, 700])
def test_gauss_chunk_boundaries(ctx, run):
    """The run a block stages for one cell row is one point short of a chunk, a chunk, one more, two chunks, two and one,
    and two and a part."""
    rng = np.random.default_rng(run)
    cloud = _packed_cloud(rng, run, 2)
    tx, ty = _targets_around_cell_33(rng, 96)
    runs = cloud.block_runs(tx, ty)
    assert len(runs) == 1 and sorted(runs[0]) == [1, 2, 3, 4, 5]
    assert runs[0][3] == run and all(v == 15 for k, v in runs[0].items() if k != 3)
    assert cloud.count(3, 3) == run - 12
    got = _gauss(ctx, cloud, tx, ty)
    _, n_acc, hits = _check_gauss(got, cloud, tx, ty)
    assert n_acc.max() > run - 60 and not hits.any()              # some target has nearly the whole packed cell in reach


def test_gauss_nan_months_across_chunks(ctx):
    """Per-chunk NaN flags: a month-1 NaN at the last slot of the first chunk and one in the second chunk only, the points
    in the same slots of the neighbouring chunks valid."""
    rng = np.random.default_rng(600)
    cloud = _packed_cloud(rng, 600, 3)
    tx, ty = _targets_around_cell_33(rng, 128)
    runs = cloud.block_runs(tx, ty)
    assert len(runs) == 1 and runs[0][3] == 600                   # chunks of 256, 256 and 88 points
    p_lo = int(cloud.cell_start[3 * 6 + 1])
    a, b = p_lo + CHUNK - 1, p_lo + CHUNK + 17
    sv = cloud.sv.copy()
    assert not np.isnan(sv).any()
    sv[a, 1] = sv[b, 1] = np.nan
    for other in (p_lo + 2 * CHUNK - 1, p_lo + 17, p_lo + 2 * CHUNK + 17):   # slot 255 of chunk 2, slot 17 of chunks 1 and 3
        assert p_lo <= other < p_lo + 600 and not np.isnan(sv[other]).any()
    clean = _gauss(ctx, cloud, tx, ty)
    got = _gauss(ctx, cloud, tx, ty, sv=sv)
    _, n_clean, _ = _check_gauss(clean, cloud, tx, ty)
    _, n_acc, _ = _check_gauss(got, cloud, tx, ty, sv=sv)
    for m in (0, 2):
        _assert_same_bits(got[m], clean[m], 'month %d next to a NaN month' % m)
        np.testing.assert_array_equal(n_acc[m], n_clean[m])
    lost = n_clean[1] - n_acc[1]
    assert lost.max() == 2 and (lost == 2).sum() >= 10 and (lost == 1).sum() >= 5    # both points matter, together and alone
    assert (got[1][lost > 0] != clean[1][lost > 0]).all()
    _assert_same_bits(got[1][lost == 0], clean[1][lost == 0], 'targets out of reach of both NaN points')


@pytest.mark.parametrize('nm', [1, 2, 3, 15, 16])
def test_gauss_number_of_fields(ctx, nm):
    """The kernel is instantiated for 16 fields (its LDS rows are 16 wide); `sval` is [nsrc][nm] packed."""
    rng = np.random.default_rng(100 + nm)
    sx, sy, sv = _background(rng, 10, nm, nan_fraction=0.05)
    sv[::37] = np.nan                                             # points that are NaN in every field
    cloud = Cloud(sx, sy, sv)
    tx, ty = rng.uniform(-1.2, 7.2, 300), rng.uniform(-1.2, 7.2, 300)
    assert len(cloud.block_runs(tx, ty)) == 2
    got = _gauss(ctx, cloud, tx, ty)
    ref, n_acc, _ = _check_gauss(got, cloud, tx, ty)
    assert got.shape == (nm, 300) and (nm == 1 or (n_acc[0] != n_acc[nm - 1]).any())     # each field has its own NaN points
    assert (n_acc.max(axis=0) == 0).sum() >= 3 and (n_acc.min(axis=0) > 0).sum() >= 200


def test_gauss_argument_errors(ctx):
    rng = np.random.default_rng(7)
    cloud = Cloud(*_background(rng, 4, 2))
    tx, ty = rng.uniform(0.0, 6.0, 50), rng.uniform(0.0, 6.0, 50)
    good = _gauss(ctx, cloud, tx, ty)
    for kw, text in [(dict(nfield=0), 'pgw_gauss_interp: nfield must be in [1, 16]'),
                     (dict(nfield=17), 'pgw_gauss_interp: nfield must be in [1, 16]'),
                     (dict(cell=np.nextafter(1.0, 0.0)),
                      'pgw_gauss_interp: cells must be at least one kernel radius wide (3 x 3 block search)')]:
        with pytest.raises(ValueError) as e:
            _gauss(ctx, cloud, tx, ty, **kw)
        assert str(e.value) == text
        _assert_same_bits(_gauss(ctx, cloud, tx, ty), good, 'first call after the error')
    _check_gauss(good, cloud, tx, ty)


def _hit_edge_offsets(x):
    """k such that a target at x + k ulp(x) is the last one coincident with a point at x (d2 < 256 eps), and k + 1 the first
    one that is not."""
    ulp = np.spacing(x)
    k = int(np.sqrt(HIT_TOL) / ulp)
    while (k * ulp) * (k * ulp) < HIT_TOL:
        k += 1
    while not (k * ulp) * (k * ulp) < HIT_TOL:
        k -= 1
    return k, k + 1, ulp


def test_gauss_exact_hits(ctx):
    rng = np.random.default_rng(8)
    bx, by, bv = _background(rng, 5, 3)
    k_in, k_out, ulp = _hit_edge_offsets(1.5)
    px = np.array([2.5, 4.25, 4.25, 1.5])
    py = np.array([2.5, 1.75, 1.75, 4.5])
    pv = np.array([[1.5, np.nan, -2.5], [3.0, -4.0, 5.0], [-30.0, 40.0, -50.0], [0.75, -0.5, 0.25]])
    cloud = Cloud(np.concatenate([bx, px]), np.concatenate([by, py]), np.concatenate([bv, pv]))
    tx, ty = rng.uniform(0.0, 6.0, 70), rng.uniform(0.0, 6.0, 70)
    tx[:4] = [2.5, 4.25, 1.5 + k_in * ulp, 1.5 + k_out * ulp]
    ty[:4] = [2.5, 1.75, 4.5, 4.5]
    # the intended conditions: the two coincident points are handed over in the order given, the first one first
    pair = np.flatnonzero((cloud.sx == 4.25) & (cloud.sy == 1.75))
    assert len(pair) == 2 and pair[1] == pair[0] + 1 and cloud.sv[pair[0], 0] == 3.0 and cloud.sv[pair[1], 0] == -30.0
    d_in, d_out = tx[2] - 1.5, tx[3] - 1.5
    assert d_in == k_in * ulp and d_out == k_out * ulp and d_in * d_in < HIT_TOL <= d_out * d_out
    got = _gauss(ctx, cloud, tx, ty)
    ref, n_acc, hits = _check_gauss(got, cloud, tx, ty)
    np.testing.assert_array_equal(hits[:, :4], [[True, True, True, False], [False, True, True, False], [True, True, True, False]])
    assert not hits[:, 4:].any()
    _assert_same_bits(got[:, 0][[0, 2]], np.array([1.5, -2.5]))              # the point's value; month 1 is the mean of the others
    assert not np.isnan(got[1, 0]) and n_acc[1, 0] == n_acc[0, 0] - 1 and n_acc[1, 0] >= 3
    _assert_same_bits(got[:, 1], np.array([3.0, -4.0, 5.0]))                 # the first of the two coincident points
    _assert_same_bits(got[:, 2], np.array([0.75, -0.5, 0.25]))               # d2 just below 256 eps
    assert (got[:, 3] != np.array([0.75, -0.5, 0.25])).all()                 # d2 just above: a weighted mean


def test_gauss_radius_edge(ctx):
    """d2 == r2 and r2 - 1 ulp are inside, r2 + 1 ulp is not.  Radius 1.4375: its neighbours in float64 square to the
    neighbours of r2 (with radius 1 no float64 squares to 1 - 2^-53).  Target and source share the other coordinate, so d2 is
    the square of one exact difference."""
    radius, h = 1.4375, 2.0
    r2 = radius * radius
    d_at, d_below, d_above = radius, np.nextafter(radius, 0.0), np.nextafter(radius, 2.0)
    assert d_at * d_at + 0.0 == r2 and d_below * d_below + 0.0 == np.nextafter(r2, 0.0) and d_above * d_above + 0.0 == np.nextafter(r2, 4.0)
    # target 0 sees all three; targets 1, 2, 3 (other rows of cells, 6 apart) have one neighbour each: above, at, below
    sx = np.array([d_at, d_below, d_above, d_above, d_at, d_below])
    sy = np.array([0.0, 0.0, 0.0, 6.0, 12.0, 18.0])
    sv = np.array([[1.0, -8.0], [2.0, 16.0], [1000.0, 1000.0], [5.0, 5.0], [7.0, -7.0], [-9.0, 9.0]])
    cloud = Cloud(sx, sy, sv, ncx=3, ncy=12, h=h)
    tx, ty = np.zeros(4), np.array([0.0, 6.0, 12.0, 18.0])
    for i in range(4):
        assert ((0.0 - cloud.sx) ** 2 + (ty[i] - cloud.sy) ** 2 <= 4 * r2).sum() == (3 if i == 0 else 1)
    got = _gauss(ctx, cloud, tx, ty, radius=radius)
    ref, n_acc, hits = _check_gauss(got, cloud, tx, ty, radius=radius)
    np.testing.assert_array_equal(n_acc, [[2, 0, 1, 1]] * 2)
    assert np.isnan(got[:, 1]).all() and not hits.any()
    assert abs(got[0, 0] - 1.5) < 1e-9 and abs(got[1, 0] - 4.0) < 1e-8     # the two that count, nearly equal weights


def _box_cloud(rng):
    sx, sy, sv = _background(rng, 8, 2, nan_fraction=0.04)
    empty = [(0, 0), (2, 2), (2, 3), (5, 4)]
    keep = np.ones(len(sx), dtype=bool)
    for cx, cy in empty:
        keep &= ~((np.floor(sx) == cx) & (np.floor(sy) == cy))
    cloud = Cloud(sx[keep], sy[keep], sv[keep])
    assert all(cloud.count(cx, cy) == 0 for cx, cy in empty) and cloud.count(1, 1) == 8
    return cloud


def _outside(rng, near, far):
    """`near` targets outside the grid [0, 6]^2 by less than the radius and `far` ones by several cells, on every side."""
    t = rng.uniform(0.0, 6.0, near + far)
    off = np.concatenate([rng.uniform(0.05, 0.95, near), rng.uniform(2.5, 6.0, far)])
    side = np.arange(near + far) % 4
    x = np.where(side == 0, -off, np.where(side == 1, 6.0 + off, t))
    y = np.where(side == 2, -off, np.where(side == 3, 6.0 + off, t))
    return x, y


def _box_targets(name, rng):
    if name == 'edge cells':                                      # first and last cell row and column
        tx, ty = rng.uniform(0.0, 6.0, 200), rng.uniform(0.0, 6.0, 200)
        k = np.arange(200) % 4
        tx = np.where(k == 0, rng.uniform(0.0, 1.0, 200), np.where(k == 1, rng.uniform(5.0, 6.0, 200), tx))
        ty = np.where(k == 2, rng.uniform(0.0, 1.0, 200), np.where(k == 3, rng.uniform(5.0, 6.0, 200), ty))
        return tx, ty
    if name == 'outside only':
        return _outside(rng, 40, 24)
    if name == 'outside and interior in one block':
        ox, oy = _outside(rng, 40, 24)
        tx, ty = np.concatenate([rng.uniform(1.0, 5.0, 150), ox]), np.concatenate([rng.uniform(1.0, 5.0, 150), oy])
        p = rng.permutation(len(tx))
        return tx[p], ty[p]
    if name == 'scattered block':                                 # no tiling: the box of the one block is the whole grid
        return rng.uniform(-0.5, 6.5, 256), rng.uniform(-0.5, 6.5, 256)
    if name == 'nan block':                                       # block 0 has no active target
        tx, ty = rng.uniform(0.0, 6.0, 512), rng.uniform(0.0, 6.0, 512)
        k = np.arange(256) % 3
        tx[:256][k != 1] = np.nan
        ty[:256][k != 0] = np.nan
        return tx, ty
    if name == 'nan and active mixed':
        tx, ty = rng.uniform(0.0, 6.0, 300), rng.uniform(0.0, 6.0, 300)
        tx[::3] = np.nan
        ty[1::7] = np.nan
        return tx, ty
    raise KeyError(name)


@pytest.mark.parametrize('name', ['edge cells', 'outside only', 'outside and interior in one block', 'scattered block',
                                  'nan block', 'nan and active mixed'])
def test_gauss_box_and_clamps(ctx, name):
    rng = np.random.default_rng(sum(map(ord, name)))
    cloud = _box_cloud(rng)
    tx, ty = _box_targets(name, rng)
    runs = cloud.block_runs(tx, ty)
    cx, cy = cloud.target_cells(tx, ty)
    out_of_grid = (cx < 0) | (cx > 5) | (cy < 0) | (cy > 5)
    dist = np.hypot(np.maximum(np.maximum(-tx, tx - 6.0), 0.0), np.maximum(np.maximum(-ty, ty - 6.0), 0.0))
    nan_t = np.isnan(tx) | np.isnan(ty)
    if name == 'edge cells':
        assert not out_of_grid.any() and all(((c == 0).sum() >= 40 and (c == 5).sum() >= 40) for c in (cx, cy))
    elif name.startswith('outside'):
        assert out_of_grid.sum() == 64 and (dist[out_of_grid] < 1.0).sum() == 40 and (dist > 2.5).sum() == 24
        for c in (cx, cy):
            assert c.min() <= -3 and c.max() >= 8 and (c == -1).any() and (c == 6).any()
        assert len(runs) == 1 and (out_of_grid.all() if name == 'outside only' else (~out_of_grid).sum() == 150)
    elif name == 'scattered block':
        assert len(runs) == 1 and out_of_grid.any()
        assert runs[0] == {ix: int(cloud.cell_start[(ix + 1) * 6] - cloud.cell_start[ix * 6]) for ix in range(6)}
    elif name == 'nan block':
        assert runs[0] is None and nan_t[:256].all() and not nan_t[256:].any() and len(runs) == 2
        assert np.isnan(tx[:256]).sum() < 256 and np.isnan(ty[:256]).sum() < 256       # NaN in x only, in y only, in both
    else:
        assert nan_t.sum() > 100 and (~nan_t).sum() > 100 and all(r is not None for r in runs)
    got = _gauss(ctx, cloud, tx, ty)
    ref, n_acc, _ = _check_gauss(got, cloud, tx, ty)
    assert np.isnan(got[:, nan_t | (dist > 1.0)]).all()
    assert (n_acc[0] > 0).sum() >= 20                             # and the others do get values
    if name.startswith('outside'):
        near = out_of_grid & (dist < 0.5)
        assert (~np.isnan(got[0][near])).sum() >= 10             # outside the grid, inside the reach of its points
    # empty cells inside the box: some block's box holds the empty cells (2, 2) and (2, 3)
    assert any(b is not None and b[0] <= 2 <= b[1] and b[2] <= 2 and b[3] >= 3 for b in cloud.block_runs(tx, ty, boxes=True))


@pytest.mark.parametrize('ntarg', [1, 255, 256, 257, 513])
def test_gauss_number_of_targets(ctx, ntarg):
    rng = np.random.default_rng(ntarg)
    cloud = _box_cloud(rng)
    tx, ty = rng.uniform(0.0, 6.0, ntarg), rng.uniform(0.0, 6.0, ntarg)
    assert len(cloud.block_runs(tx, ty)) == -(-ntarg // BLOCK)
    _check_gauss(_gauss(ctx, cloud, tx, ty), cloud, tx, ty)


@pytest.mark.parametrize('null_sources', [False, True], ids=['dummy source arrays', 'null source pointers'])
def test_gauss_empty_cloud(ctx, null_sources):
    """nsrc = 0 with cell_start = [0, 0] (the host's form of a cloud without a valid point): NaN everywhere."""
    rng = np.random.default_rng(3)
    cloud = Cloud(np.zeros(0), np.zeros(0), np.zeros((0, 2)), ncx=1, ncy=1)
    np.testing.assert_array_equal(cloud.cell_start, [0, 0])
    tx, ty = rng.uniform(-3.0, 3.0, 300), rng.uniform(-3.0, 3.0, 300)
    tx[5] = np.nan
    got = _gauss(ctx, cloud, tx, ty, null_sources=null_sources)
    assert got.shape == (2, 300) and np.isnan(got).all()


def test_gauss_underflow(ctx):
    """Sharpness 30: exp(-900 d2) is 0 in float64 from d = 0.91 on.  A target all of whose neighbours are that far away has
    no value, on both sides; no target of the case has ONLY subnormal weights (their relative error is not an ulp's)."""
    rng = np.random.default_rng(30)
    sx, sy, sv = _background(rng, 20, 2)
    hole = (3.0, 3.0)
    far = np.hypot(sx - hole[0], sy - hole[1]) > 1.0
    ang = np.arange(12) * (2 * np.pi / 12) + 0.1
    sx = np.concatenate([sx[far], hole[0] + 0.95 * np.cos(ang)])
    sy = np.concatenate([sy[far], hole[1] + 0.95 * np.sin(ang)])
    sv = np.concatenate([sv[far], rng.normal(0.0, 5.0, (12, 2))])
    cloud = Cloud(sx, sy, sv)
    tx, ty = rng.uniform(0.0, 6.0, 400), rng.uniform(0.0, 6.0, 400)
    tx[0], ty[0] = hole
    w_max = np.zeros(400)
    n_zero = np.zeros(400, dtype=int)
    for i in range(400):
        _, _, w = H.gauss_geometry(tx[i], ty[i], cloud.sx, cloud.sy, 1.0, 30.0)
        w_max[i], n_zero[i] = w.max(), (w == 0).sum()
    sound = (w_max == 0) | (w_max > 1e-250)
    tx, ty, w_max, n_zero = tx[sound], ty[sound], w_max[sound], n_zero[sound]
    assert sound[0] and sound.sum() >= 380 and w_max[0] == 0 and n_zero[0] == 12
    assert ((w_max > 0) & (n_zero > 0)).sum() > 300               # weights at the rim are 0, nearer ones are not
    got = _gauss(ctx, cloud, tx, ty, sharpness=30.0)
    ref, n_acc, _ = _check_gauss(got, cloud, tx, ty, sharpness=30.0)
    assert (n_acc[:, 0] == 12).all() and np.isnan(got[:, 0]).all()
    np.testing.assert_array_equal(np.isnan(got[0]), w_max == 0)


def test_gauss_order_independence(ctx):
    """A thread's sums follow its own (ix, iy, p) walk, whatever the box of its block is."""
    rng = np.random.default_rng(41)
    sx, sy, sv = _background(rng, 12, 3, nan_fraction=0.03)
    cloud = Cloud(sx, sy, sv)
    gx, gy = np.meshgrid(np.linspace(-0.4, 6.4, 25), np.linspace(-0.4, 6.4, 24), indexing='ij')
    tx, ty = gx.ravel(), gy.ravel()                               # natural order: rows of a grid, compact boxes
    perm = rng.permutation(len(tx))
    runs_nat, runs_perm = cloud.block_runs(tx, ty), cloud.block_runs(tx[perm], ty[perm])
    assert len(runs_nat) == 3 and sum(sum(r.values()) for r in runs_perm) > 1.5 * sum(sum(r.values()) for r in runs_nat)
    nat = _gauss(ctx, cloud, tx, ty)
    got = _gauss(ctx, cloud, tx[perm], ty[perm])
    back = np.empty_like(got)
    back[:, perm] = got
    _assert_same_bits(back, nat, 'natural order vs a random permutation of the targets')
    _check_gauss(nat, cloud, tx, ty)


# ------------------------------------------------------------------ gauss_interp_fields: the host branches
def _ocean_case():
    from pgw4era5_amd import synthetic
    oc = synthetic.make_ocean_grid_case(nj=18, ni=26, ntime=3, seed=2)
    lat = np.linspace(-90.0, 90.0, 13)
    lon = np.arange(20) * (360.0 / 20)
    land = (np.random.default_rng(1).uniform(size=(13, 20)) > 0.8).astype(np.float64)
    return oc, lat, lon, land


def test_gauss_interp_fields_more_than_16_fields(ctx):
    """17 fields: a second pass with a re-uploaded value slice."""
    from pgw4era5_amd import functions as F
    oc, lat, lon, land = _ocean_case()
    rng = np.random.default_rng(17)
    fields = [oc['values'][k % 3] * rng.normal() + rng.normal() * oc['values'][(k + 1) % 3] for k in range(17)]
    assert all((np.isnan(f) == np.isnan(fields[0])).all() for f in fields) and 0 < np.isnan(fields[0]).sum() < fields[0].size
    args = (land, lat, lon, oc['latitude'], oc['longitude'])
    all17 = F.gauss_interp_fields(*args, fields, 2.5e6, 4.0)
    first16 = F.gauss_interp_fields(*args, fields[:16], 2.5e6, 4.0)
    last = F.gauss_interp_fields(*args, fields[16:], 2.5e6, 4.0)
    assert all17.shape == (17, 13, 20) and 0 < np.isnan(all17[16]).sum() < 260
    _assert_same_bits(all17[:16], first16, 'fields 0 .. 15 of 17 vs a 16-field call')
    _assert_same_bits(all17[16:], last, 'field 16 of 17 vs a 1-field call')
    assert len(np.unique(all17[:, ~np.isnan(all17[0])], axis=0)) == 17


def test_gauss_interp_fields_nan_fields(ctx):
    from pgw4era5_amd import functions as F
    oc, lat, lon, land = _ocean_case()
    args = (land, lat, lon, oc['latitude'], oc['longitude'])
    # NaN everywhere: a cloud without a point
    nothing = F.gauss_interp_fields(*args, [np.full_like(oc['values'][0], np.nan)] * 2, 2.5e6, 4.0)
    assert nothing.shape == (2, 13, 20) and np.isnan(nothing).all()
    # points that are NaN in every field but one stay in the cloud for that one
    b = oc['values'][1]
    a = oc['values'][0].copy()
    a[3:9, 5:15] = np.nan
    assert (np.isnan(a) & ~np.isnan(b)).sum() >= 30 and not (np.isnan(b) & ~np.isnan(a)).any()
    both = F.gauss_interp_fields(*args, [a, a * 2.0, b], 2.5e6, 4.0)
    alone = F.gauss_interp_fields(*args, [b], 2.5e6, 4.0)
    _assert_same_bits(both[2], alone[0], 'the one field that has the points')
    plain = F.gauss_interp_fields(*args, [oc['values'][0]], 2.5e6, 4.0)
    assert np.nanmax(np.abs(both[0] - plain[0])) > 1e-6           # and the fields without them do not see them


# ------------------------------------------------------------------ pgw_harmonic_smooth
NTIMES = [8, 9, 15, 16, 17, 365, 366, 1365]
INNERS = [1, 63, 64, 65, 255, 256, 257, 513]
SHAPES = sorted(set([(nt, 257) for nt in NTIMES] + [(17, n) for n in INNERS] + [(1365, 65)]))


def _smooth(ctx, x):
    from pgw4era5_amd import functions as F
    from pgw4era5_amd.device import dtype_tag
    x = np.ascontiguousarray(x)
    ntime, inner = x.shape
    cos_t, sin_t = F.harmonic_tables(ntime)
    assert cos_t.shape == sin_t.shape == (3, ntime) and cos_t.flags.c_contiguous and sin_t.flags.c_contiguous
    d_in = ctx.to_device(x)
    d_out = ctx.to_device(np.full(x.shape, SENTINEL, dtype=x.dtype))
    ctx._check(ctx.lib.pgw_harmonic_smooth(ctx.handle, dtype_tag(x.dtype), ntime, inner, cos_t.ctypes.data_as(_dp),
                                           sin_t.ctypes.data_as(_dp), d_in.ptr, d_out.ptr))
    out = d_out.numpy()
    assert out.dtype == x.dtype and out.shape == x.shape
    return out


def _check_smooth(got, x, ref=None):
    """got against harmonic_reference(x) (or `ref`) with the bound of the module docstring, per column."""
    ref = H.harmonic_reference(x) if ref is None else ref
    nan = np.isnan(ref)
    np.testing.assert_array_equal(np.isnan(got), nan)
    ntime = x.shape[0]
    col = ~nan.any(axis=0)
    bound = np.broadcast_to(13 * (ntime + 4) * LD(EPS) * np.abs(x[:, col].astype(LD)).max(axis=0), ref[:, col].shape)
    if got.dtype == np.float32:
        bound = bound + LD(2.0 ** -24) * np.abs(ref[:, col])
    err = np.abs(got[:, col].astype(LD) - ref[:, col])
    assert (err <= bound).all(), 'worst %.3f of the bound' % float((err / bound).max())
    _record('k_harmonic_smooth %s' % got.dtype, err, bound)


def _nan_placements(ntime, inner):
    """{column: step}: a NaN in the first step only, in the last step only (the unroll tail re-reads the last row), in
    column inner - 1, in column 0 of the second block; their neighbours stay valid."""
    if inner < 8:
        return {inner - 1: ntime - 1}
    place = {1: 0, 3: ntime - 1, inner - 1: ntime // 2}
    if inner > BLOCK:
        place[BLOCK] = 2
    return place


@pytest.mark.parametrize('dtype', ['float64', 'float32'])
@pytest.mark.parametrize('shape', SHAPES, ids=['%dx%d' % s for s in SHAPES])
def test_harmonic_smooth_shapes_and_nan_columns(ctx, shape, dtype):
    ntime, inner = shape
    rng = np.random.default_rng(ntime * 1000 + inner)
    x = rng.normal(250.0, 20.0, shape).astype(dtype)
    if dtype == 'float32':                                        # values whose sums are not float32 numbers
        assert (x.astype(np.float64).sum(axis=0) != x.sum(axis=0, dtype=np.float32)).any() or inner == 1
    clean = _smooth(ctx, x)
    _check_smooth(clean, x)
    place = _nan_placements(ntime, inner)
    xn = x.copy()
    for c, t in place.items():
        xn[t, c] = np.nan
    assert np.isnan(xn).sum() == len(place) and (inner < 8 or {0, 2, 4, inner - 2} & set(place) == set())
    assert inner <= BLOCK or ({BLOCK - 1, BLOCK + 1} & set(place) == set() and BLOCK in place)
    got = _smooth(ctx, xn)
    cols = sorted(place)
    assert np.isnan(got[:, cols]).all()
    rest = np.ones(inner, dtype=bool)
    rest[cols] = False
    _assert_same_bits(got[:, rest], clean[:, rest], 'columns next to a NaN column')


@pytest.mark.parametrize('dtype', ['float64', 'float32'])
@pytest.mark.parametrize('ntime', [8, 17, 365, 366])
def test_harmonic_smooth_returns_a_harmonic_series(ctx, ntime, dtype):
    """A series that is exactly mean + three harmonics comes back.  float64: within the bound of the series itself (the
    reference of such a series is the series to 1e-13 of its scale, tests/test_step02_kernels_host.py).  float32: the
    rounded series is no longer a sum of harmonics, so it is held to the reference of the rounded series."""
    x = H.harmonic_series(ntime, 65, ntime)
    got = _smooth(ctx, x.astype(dtype))
    if dtype == 'float64':
        _check_smooth(got, x, ref=x.astype(LD))
    _check_smooth(got, x.astype(dtype))


@pytest.mark.parametrize('dtype', ['float64', 'float32'])
def test_harmonic_smooth_argument_errors(ctx, dtype):
    rng = np.random.default_rng(5)
    x = rng.normal(250.0, 20.0, (1366, 5)).astype(dtype)
    good = _smooth(ctx, x[:1365])
    _check_smooth(good, x[:1365])
    for ntime, text in [(7, 'Whooops that should not be the case for a yearly timeseries! i (reconstruction grade) is larger '
                            'than the number of timeseries elements / 2.'),
                        (1366, 'pgw_harmonic_smooth: time series longer than 1365 steps are not supported')]:
        with pytest.raises(ValueError) as e:
            _smooth(ctx, x[:ntime])
        assert str(e.value) == text
        _assert_same_bits(_smooth(ctx, x[:1365]), good, 'first call after the error')


# ------------------------------------------------------------------ pgw_planar_metres
def test_planar_metres_keeps_nan_points_to_themselves(ctx):
    """A NaN latitude or longitude gives NaN in lon_m (and in lat_m for a NaN latitude); every other point is the bits of a
    run without the NaN points."""
    from pgw4era5_amd import functions as F
    rng = np.random.default_rng(14)
    n = 600
    lat, lon = rng.uniform(-89.0, 89.0, n), rng.uniform(-179.0, 179.0, n)
    clean = F.planar_metres(lat, lon)
    assert not any(np.isnan(c).any() for c in clean)
    lat2, lon2 = lat.copy(), lon.copy()
    nan_lat, nan_lon, nan_both = [5, 64, 255, 599], [0, 63, 256, 300], [17]
    lat2[nan_lat + nan_both] = np.nan
    lon2[nan_lon + nan_both] = np.nan
    got = F.planar_metres(lat2, lon2)
    assert np.isnan(got[1][nan_lat + nan_lon + nan_both]).all() and np.isnan(got[0][nan_lat + nan_both]).all()
    other = np.ones(n, dtype=bool)
    other[nan_lat + nan_lon + nan_both] = False
    for g, c, name in zip(got, clean, ('lat_m', 'lon_m', 'lon_off')):
        _assert_same_bits(g[other], c[other], name)
    _assert_same_bits(got[0][nan_lon], clean[0][nan_lon], 'lat_m of a NaN longitude')
    _assert_same_bits(got[2][nan_lon], clean[2][nan_lon], 'lon_off of a NaN longitude')
