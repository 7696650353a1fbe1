"""`pgw_regrid_bilinear` (k_regrid, k_zonal_mean_rows) at its window, slice and pole edges, called directly through the C
API into an output prefilled with a sentinel, and through `functions.regrid_field`.

The cases, their own conditions, the longdouble reference and the float64 restatement of the kernel are those of
tests/test_regrid_edges_host.py; the tolerances are derived in its docstring.  In short, per output value:

  bits      float64 and float32, no pole row in the target's stencil: the bits of `kernel_statement` (the same IEEE
            operations in the same order; the float32 result is its float64 value rounded once).
  bound     everywhere, against the longdouble reference: 4 eps (|y_lo| + |y_hi|) per interpolation, carried through the
            two passes; a pole row enters with (n - 1) eps sum|v| / n + eps |mean| (its zonal mean summed in any order,
            one division); float32 adds 2^-24 |ref|.
  NaN       masks equal the reference's, exactly.

No element of the output may keep the sentinel.  The largest observed error of each group as a fraction of its bound is
printed at the end of the module (run with -s)."""
import ctypes as C

import numpy as np
import pytest

import test_regrid_edges_host as H
from test_regrid_edges_host import LD

pytestmark = pytest.mark.gpu

_dp, _ip = C.POINTER(C.c_double), C.POINTER(C.c_int)
SENTINEL = -777.0                 # what the output holds before a call: every element must be overwritten
WORST = {}                        # group -> largest observed error / bound
BITS = {'compared': 0, 'different': 0}
DTYPES = ['float64', 'float32']
PGW_ERR_ARG = 2


@pytest.fixture(scope='module')
def ctx():
    from pgw4era5_amd.device import default_context
    yield default_context()
    if WORST:
        print('\nlargest observed error as a fraction of the derived bound: ' +
              ', '.join('%s %.3f' % kv for kv in sorted(WORST.items())))
        print('values compared by their bits with the float64 restatement of the kernel: %(compared)d, different: %(different)d' % BITS)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype == np.float64 else np.uint32)


def _record(name, err, bound):
    pos = bound > 0
    if pos.any():
        WORST[name] = max(WORST.get(name, 0.0), float((err[pos] / bound[pos]).max()))


def _call(ctx, field, tb, force_vec1=False, south_row=None, north_row=None, out=None):
    """One pgw_regrid_bilinear call on tables `tb`; returns (status, output as (nfield, nlat_t, nlon_t))."""
    from pgw4era5_amd.device import dtype_tag
    field = np.ascontiguousarray(field)
    nlat_s, nlon_s = field.shape[-2:]
    nfield = int(np.prod(field.shape[:-2], dtype=np.int64))
    t = {k: np.ascontiguousarray(v) for k, v in tb.items() if isinstance(v, np.ndarray)}
    nlat_t, nlon_t = len(t['lat_lo']), len(t['lon_lo'])
    for k in ('lat_lo', 'lat_hi', 'lat_oob', 'lon_lo', 'lon_hi', 'lon_oob'):
        assert t[k].dtype == np.int32
    d_src = ctx.to_device(field)
    d_out = ctx.to_device(np.full((nfield, nlat_t, nlon_t), SENTINEL, dtype=field.dtype)) if out is None else out
    old = ctx.set_option('force_vec1', 1 if force_vec1 else 0)
    try:
        rc = ctx.lib.pgw_regrid_bilinear(
            ctx.handle, dtype_tag(field.dtype), nfield, nlat_s, nlon_s, nlat_t, nlon_t, d_src.ptr,
            t['lat_lo'].ctypes.data_as(_ip), t['lat_hi'].ctypes.data_as(_ip), t['lat_dx'].ctypes.data_as(_dp),
            t['lat_Dx'].ctypes.data_as(_dp), t['lat_oob'].ctypes.data_as(_ip),
            t['lon_lo'].ctypes.data_as(_ip), t['lon_hi'].ctypes.data_as(_ip), t['lon_dx'].ctypes.data_as(_dp),
            t['lon_Dx'].ctypes.data_as(_dp), t['lon_oob'].ctypes.data_as(_ip),
            tb['south_row'] if south_row is None else south_row, tb['north_row'] if north_row is None else north_row, d_out.ptr)
    finally:
        ctx.set_option('force_vec1', old)
    return rc, d_out.numpy()


def _run(ctx, c, dtype, tb=None):
    rc, got = _call(ctx, c.typed(dtype), c.tb if tb is None else tb, c.force_vec1)
    ctx._check(rc)
    assert got.dtype == np.dtype(dtype) and got.shape == (c.nfield, c.nlat_t, c.nlon_t)
    assert (got != SENTINEL).all(), '%d elements were not written' % int((got == SENTINEL).sum())
    return got


def _check(c, got, dtype):
    """got (nfield, nlat_t, nlon_t) against the reference (mask, bound) and, away from the pole rows, against the bits of
    the kernel's restatement."""
    ref, bound = c.reference(dtype)
    ref, bound = ref.reshape(got.shape), bound.reshape(got.shape)
    nan = np.isnan(ref)
    np.testing.assert_array_equal(np.isnan(got), nan, err_msg='NaN mask')
    err = np.abs(got.astype(LD) - ref)
    for rows, name in ((~c.pole_rows, 'no pole row'), (c.pole_rows, 'pole row')):
        ok = ~nan[:, rows, :]
        if not ok.any():
            continue
        e, b = err[:, rows, :][ok], bound[:, rows, :][ok]
        print('%s %s: largest error / bound %.3f over %d values' % (dtype, name, float((e / b).max()), e.size))
        _record('%s %s' % (dtype, name), e, b)
        assert (e <= b).all(), '%s, %s: %d of %d values beyond the bound, worst %.3f of it' % (dtype, name, int((e > b).sum()), e.size,
                                                                                             float((e / b).max()))
    want = H.kernel_statement(c.typed(dtype), c.tb, c.numpy_poles(dtype))
    away = ~c.pole_rows
    a, b = _bits(got[:, away, :]), _bits(want[:, away, :])
    both_nan = np.isnan(got[:, away, :]) & np.isnan(want[:, away, :])
    diff = (a != b) & ~both_nan
    BITS['compared'] += int(a.size)
    BITS['different'] += int(diff.sum())
    print('%s bits away from the pole rows: %d compared, %d different' % (dtype, a.size, int(diff.sum())))
    assert not diff.any(), '%d of %d values differ in their bits from the restatement of the kernel' % (int(diff.sum()), a.size)
    return ref


# ------------------------------------------------------------------ cases 1 - 7
WINDOW = ['window 765', 'window 768', 'window 765 vec1', 'window 765 odd']
SEAM = ['gap W2', 'gap W1', 'seam mid block', 'seam staged W2']
ORDER = ['descending source', 'descending targets', 'descending both', 'unsorted duplicate targets']


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('name', WINDOW + SEAM)
def test_windows_at_the_tile_boundary_and_the_seam(ctx, name, dtype):
    """Cases 1 and 2: spans of 256 and 257 in one launch, all above, all below (W = 1); a block that starts in the periodic
    gap; a staged window that runs over the seam."""
    c = H.get_case(name)
    _check(c, _run(ctx, c, dtype), dtype)


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('nfield', H.SLICE_NFIELDS)
def test_plane_slices(ctx, nfield, dtype):
    """Case 3: 1, 7, 8, 9, 16 planes in one-plane slices with and without the interleaved decode; 19: slices of 3, one of
    1 and an empty one; 40: slices of 5 = FU + 1.  Every plane is its own, about 100 apart."""
    c = H.get_case('slices %d' % nfield)
    got = _run(ctx, c, dtype)
    ref = _check(c, got, dtype)
    mid = np.nanmean(got.astype(np.float64), axis=(1, 2))
    np.testing.assert_allclose(mid, 100.0 * (1 + np.arange(nfield)), atol=20.0)           # plane k from source plane k
    assert ref.shape == got.shape
    if nfield == 1:                                                # a 2-D field through the function-level entry
        from pgw4era5_amd import functions as F
        f2 = c.typed(dtype)
        assert f2.ndim == 2
        out = np.asarray(F.regrid_field(f2, c.src_lat, c.src_lon, c.targ_lat, c.targ_lon))
        assert out.shape == (c.nlat_t, c.nlon_t) and out.dtype == np.dtype(dtype)
        np.testing.assert_array_equal(_bits(out), _bits(got[0]))


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('name', H.POLE_CASES)
def test_poles(ctx, name, dtype):
    """Case 4: one pole only, none (k_zonal_mean_rows not launched), pole rows from partly and all NaN source rows, the
    source's own -90 next to the reference's pole row (x_hi - x_lo == 0: NaN in that target row alone) - through the C API
    and through regrid_field, which give the same bits."""
    from pgw4era5_amd import functions as F
    c = H.get_case(name)
    got = _run(ctx, c, dtype)
    ref = _check(c, got, dtype)
    if name == 'pole in source':
        assert np.isnan(got[:, 0, :]).all() and not np.isnan(got[:, 1:, :]).any()
    else:
        pr = c.pole_rows
        assert not np.isnan(got[0]).any() and not np.isnan(got[3]).any()
        if pr.any():                                               # plane 1: a mean of the valid values; plane 2: none
            assert np.isnan(ref[1][pr]).any() and not np.isnan(got[1][pr]).all() and np.isnan(got[2][pr]).all()
    out = np.asarray(F.regrid_field(c.typed(dtype), c.src_lat, c.src_lon, c.targ_lat, c.targ_lon))
    assert out.shape == c.field.shape[:-2] + (c.nlat_t, c.nlon_t) and out.dtype == np.dtype(dtype)
    a, b = _bits(out.reshape(got.shape)), _bits(got)
    assert ((a == b) | (np.isnan(out.reshape(got.shape)) & np.isnan(got))).all()


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('name', ORDER + ['regional nodes', 'both extensions'])
def test_row_order_nodes_and_extensions(ctx, name, dtype):
    """Cases 5 - 7: un-flipped rows of a descending source, descending / unsorted / duplicate targets; a regional source
    with targets on its nodes and a NaN neighbour of weight 0; both +-360 copies at once."""
    c = H.get_case(name)
    got = _run(ctx, c, dtype)
    ref = _check(c, got, dtype)
    if name == 'regional nodes':
        assert np.isnan(got[0, 5, 7]) and np.isnan(got[0, 4, 8]) and np.isnan(got[1, 0, 0]) and not np.isnan(got[0, 3, 7])
    if name == 'unsorted duplicate targets':
        for v in (0.0, 123.6):                                     # a duplicate target is the same value again
            same = np.flatnonzero(c.targ_lon == v)
            assert len(same) >= 2
            for s in same[1:]:
                np.testing.assert_array_equal(_bits(got[:, :, s]), _bits(got[:, :, same[0]]))
        np.testing.assert_array_equal(_bits(got[:, 0, :]), _bits(got[:, 3, :]))            # the duplicate target latitude
    assert ref.shape == got.shape


# ------------------------------------------------------------------ case 8: lat_oob / lon_oob of the C ABI
@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('force_vec1', [False, True], ids=['W2', 'W1'])
def test_oob_flags(ctx, force_vec1, dtype):
    """NaN exactly at the flagged rows and columns, the bits of the unflagged call elsewhere: a block without a valid
    target, a block whose first valid target is not its first, flagged columns in staged and direct blocks, flagged rows
    (direct gathers, nothing read)."""
    c, tb = H.case_oob(force_vec1)
    clean = _run(ctx, c, dtype)
    got = _run(ctx, c, dtype, tb=tb)
    flagged = np.zeros(got.shape, dtype=bool)
    flagged[:, tb['lat_oob'] != 0, :] = True
    flagged[:, :, tb['lon_oob'] != 0] = True
    assert not np.isnan(clean).any()
    np.testing.assert_array_equal(np.isnan(got), flagged)
    np.testing.assert_array_equal(_bits(got[~flagged]), _bits(clean[~flagged]))
    _check(c, clean, dtype)


# ------------------------------------------------------------------ case 9: validation
@pytest.mark.parametrize('which', ['lat_lo south', 'lat_hi south', 'lat_lo north', 'lat_hi north'])
def test_pole_rows_in_the_tables_need_their_source_row(ctx, which):
    """Tables that name row -1 (nlat_s) while south_row (north_row) is -1: an argument error before any upload or launch -
    the pole values would be whatever the workspace held.  The same entries under lat_oob are not read and pass."""
    c = H.get_case('pole none')
    key, side = which.split()
    tb = H.oob_tables(c, [], [])
    tb[key][2] = -1 if side == 'south' else c.nlat_s
    assert tb['south_row'] == tb['north_row'] == -1
    field = c.typed('float64')
    d_out = ctx.to_device(np.full((c.nfield, c.nlat_t, c.nlon_t), SENTINEL))
    ctx.profile(True)
    ctx.profile_reset()
    try:
        rc, out = _call(ctx, field, tb, out=d_out)
        launches = ctx.profile_get('regrid')[0]
    finally:
        ctx.profile(False)
    assert rc == PGW_ERR_ARG, 'status %d for tables that name a pole row nobody computes' % rc
    assert launches == 0 and (out == SENTINEL).all()
    with pytest.raises(ValueError) as e:
        ctx._check(rc)
    assert 'pole row' in str(e.value) and e.value.status == PGW_ERR_ARG
    # with the source row named, the same tables are served; flagged out of bounds, they are not read
    other = dict(south_row=0) if side == 'south' else dict(north_row=c.nlat_s - 1)
    ctx.profile(True)
    ctx.profile_reset()
    try:
        rc, out = _call(ctx, field, tb, **other)
        launches = ctx.profile_get('regrid')[0]
    finally:
        ctx.profile(False)
    assert launches == 1                                          # what the 0 above is counted in: one timed scope per call
    assert rc == 0 and (out != SENTINEL).all() and not np.isnan(out[0]).any()
    tb['lat_oob'][2] = 1
    rc, out = _call(ctx, field, tb)
    assert rc == 0 and (out != SENTINEL).all() and np.isnan(out[:, 2, :]).all()
    _check(c, _run(ctx, c, 'float64'), 'float64')                 # and the context serves the next call


def test_argument_errors_leave_the_output_alone(ctx):
    """The sibling of tests/test_regrid_points_hip.py::test_argument_errors_leave_the_output_alone: every argument error of
    pgw_regrid_bilinear is PGW_ERR_ARG with the output untouched; out-of-range entries under lat_oob / lon_oob are not read."""
    from pgw4era5_amd import _lib
    c = H.Case(H._field(np.random.default_rng(58), (3, 5, 8)), np.array([-72.0, -36.5, 0.0, 36.5, 72.0]), np.arange(8) * 45.0,
               np.array([-90.0, -40.5, 10.2, 80.0]), np.array([0.0, 50.5, 133.0, 200.2, 310.0, 359.0]))
    assert c.tb['south_row'] == 0 and c.tb['north_row'] == 4 and c.pole_rows.tolist() == [True, False, False, True]
    src = ctx.to_device(c.field)
    sentinel = np.full((3, 4, 6), SENTINEL)
    out = ctx.to_device(sentinel)
    base = {k: np.ascontiguousarray(v) for k, v in c.tb.items() if isinstance(v, np.ndarray)}

    def rc(dtype=_lib.PGW_F64, nfield=3, nlat_s=5, nlon_s=8, nlat_t=4, nlon_t=6, s=src.ptr, o=out.ptr, south=0, north=4, null=None, **edit):
        t = {k: v.copy() for k, v in base.items()}
        for k, (i, v) in edit.items():
            t[k][i] = v
        p = {k: (None if k == null else v.ctypes.data_as(_ip if v.dtype == np.int32 else _dp)) for k, v in t.items()}
        return ctx.lib.pgw_regrid_bilinear(ctx.handle, dtype, nfield, nlat_s, nlon_s, nlat_t, nlon_t, s, p['lat_lo'], p['lat_hi'],
                                           p['lat_dx'], p['lat_Dx'], p['lat_oob'], p['lon_lo'], p['lon_hi'], p['lon_dx'], p['lon_Dx'],
                                           p['lon_oob'], south, north, o)
    bad = [rc(dtype=7), rc(nfield=0), rc(nlat_s=1), rc(nlon_t=0), rc(s=None), rc(o=None), rc(null='lat_hi'), rc(null='lon_dx'),
           rc(lat_lo=(1, -2)), rc(lat_hi=(1, 6)), rc(lon_lo=(2, -1)), rc(lon_hi=(2, 8)), rc(south=5), rc(north=5)]
    assert bad == [PGW_ERR_ARG] * len(bad), bad
    ctx.sync()
    np.testing.assert_array_equal(out.numpy(), sentinel)                             # nothing ran
    with pytest.raises(ValueError, match='pgw_regrid_bilinear'):
        ctx._check(rc(lat_lo=(1, -2)))
    # the same entries in a flagged row / column are not read
    assert rc(lat_oob=(1, 1), lat_lo=(1, -2), lat_hi=(1, 6), lon_oob=(2, 1), lon_lo=(2, -1), lon_hi=(2, 8)) == _lib.PGW_OK
    flagged = np.zeros(sentinel.shape, dtype=bool)
    flagged[:, 1, :] = flagged[:, :, 2] = True
    np.testing.assert_array_equal(np.isnan(out.numpy()), flagged)
    assert rc() == _lib.PGW_OK
    _check(c, out.numpy(), 'float64')
