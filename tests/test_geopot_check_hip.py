"""GPU tests of the hydrostatic check: `pgw_geopot_on_plev` (k_geopot_plev) through functions.geopot_on_plev /
geopot_change_on_plev, `pgw_level_stats` (k_level_stats), and check_geopot.check_file with its command line, against the
numpy statement of tests/geopot_statement.py (checked on the CPU by tests/test_geopot_check_host.py).

Bounds.  phi against the statement: rtol = 1e-9, the project's RT for integ_geopot (the kernel's table logarithm against
numpy's).  A difference of two such values: atol = 1e-9 * max|phi|.  NaN masks and NaN counts: equal.  What is arithmetic
on the same values in the same order - the two-state forms against the composed one-state calls, level orders against each
other, a level that equals a half-level pressure - is asserted bit for bit."""
import datetime as dt
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import geopot_statement as G                                                         # noqa: E402
from oracle import pgw_oracle as O                                                   # noqa: E402
from pgw4era5_amd import synthetic                                                   # noqa: E402

pytestmark = pytest.mark.gpu

RT = 1e-9
LERP, RECORD = dt.datetime(2006, 8, 2, 3), dt.datetime(2006, 8, 15, 12)      # between two monthly records; ON the eighth
# (columns as nlat x nlon, nlev, seed): one column, less than a wave + a second wave, odd multiples, more than one block
SHAPES = [((1, 1), 21, 0), ((6, 11), 12, 3), ((8, 12), 2, 5), ((15, 20), 21, 7), ((6, 11), 1, 0), ((15, 20), 12, 5),
          ((8, 12), 21, 3), ((1, 1), 2, 7)]


@pytest.fixture(scope='module')
def F():
    from pgw4era5_amd import functions
    return functions


def bits(x):
    """The bit patterns of x with every NaN as one pattern (sign and payload of a NaN are not data)."""
    x = np.ascontiguousarray(x, dtype=np.float64)
    return np.where(np.isnan(x), np.uint64(0x7ff8000000000000), x.view(np.uint64))


@functools.lru_cache(maxsize=None)
def case(grid, nlev, seed, dtype='float64', target=LERP):
    return synthetic.make_case(nlat=grid[0], nlon=grid[1], nlev=nlev, seed=seed, dtype=np.dtype(dtype), target_dt=target)


@functools.lru_cache(maxsize=None)
def statement(grid, nlev, seed, dtype='float64'):
    """phi on PLEV19 + the tie level (20 levels, descending then the tie level) of the ERA state; read-only."""
    era = case(grid, nlev, seed, dtype)['era']
    plev = levels20(era)
    phi = G.phi_on_plev(era['PS'], era['FIS'], era['T'], era['QV'], era['ak'], era['bk'], plev)
    phi.setflags(write=False)
    return plev, phi


def levels20(era):
    plev = np.concatenate([synthetic.PLEV19, [G.tie_level(era['ak'], era['bk'])[0]]])
    return plev[plev > 0.0001]                      # nlev = 1: the only pure-pressure half level is the top, ak = 0


def one_state(F, era, plev):
    return F.geopot_on_plev(era['PS'], era['FIS'], era['T'], era['QV'], era['ak'], era['bk'], plev, counts=True)


# ---- 1. one state against the statement ----------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', ['float64', 'float32'])
@pytest.mark.parametrize('grid,nlev,seed', SHAPES)
def test_one_state_against_the_statement(F, grid, nlev, seed, dtype):
    era = case(grid, nlev, seed, dtype)['era']
    plev, want = statement(grid, nlev, seed, dtype)
    got, nan = one_state(F, era, plev)
    assert got.dtype == np.float64 and got.shape == want.shape
    assert np.array_equal(np.isnan(got), np.isnan(want))
    np.testing.assert_allclose(got, want, rtol=RT, atol=0.0, equal_nan=True)
    assert nan.tolist() == np.isnan(want).sum(axis=(0, 2, 3)).tolist()
    share = np.isnan(got).mean()
    print('%s columns=%d nlev=%d: NaN share %.4f' % (dtype, grid[0] * grid[1], nlev, share))
    assert share <= 0.10                                           # a kernel cannot pass by returning NaN
    assert not np.isnan(got[0, list(plev).index(50000.0):19]).any()


@pytest.mark.parametrize('dtype', ['float64', 'float32'])
def test_level_lists_and_orders(F, dtype):
    """S = 1, 2, 19, 20 (with the tie level); descending, ascending and shuffled lists give the same rows, bit for bit."""
    grid, nlev, seed = (15, 20), 21, 7
    era = case(grid, nlev, seed, dtype)['era']
    plev, want = statement(grid, nlev, seed, dtype)
    full, nan_full = one_state(F, era, plev)
    rng = np.random.default_rng(1)
    orders = dict(ascending=np.argsort(plev), shuffled=rng.permutation(len(plev)), nineteen=np.arange(19), two=np.array([7, 2]),
                  one=np.array([19]), one_low=np.array([0]), repeated=np.array([3, 3, 11]))
    for name, idx in orders.items():
        got, nan = one_state(F, era, plev[idx])
        assert np.array_equal(bits(got), bits(full[:, idx])), name
        assert nan.tolist() == nan_full[idx].tolist(), name
        np.testing.assert_allclose(got, want[:, idx], rtol=RT, atol=0.0, equal_nan=True, err_msg=name)


@pytest.mark.parametrize('dtype', ['float64', 'float32'])
def test_edge_columns(F, dtype):
    """PS on a level (FIS exactly), one ulp beside it, the tie level, a column that does not ascend, a NaN PS - alone (every
    wave takes the general form) and appended to ascending columns."""
    e = G.edge_case(np.dtype(dtype))
    want = G.phi_on_plev(e['ps'], e['fis'], e['ta'], e['hus'], e['ak'], e['bk'], e['plev'])
    got, nan = F.geopot_on_plev(e['ps'], e['fis'], e['ta'], e['hus'], e['ak'], e['bk'], e['plev'], counts=True)
    assert np.array_equal(np.isnan(got), np.isnan(want))
    np.testing.assert_allclose(got, want, rtol=RT, atol=0.0, equal_nan=True)
    assert nan.tolist() == np.isnan(want).sum(axis=(0, 2, 3)).tolist()
    col = {n: i for i, n in enumerate(e['names'])}
    lev = {p: i for i, p in enumerate(e['plev'])}
    g, fis = got[0, :, 0, :], np.asarray(e['fis'], dtype=np.float64)[0, 0]
    assert g[lev[100000.0], col['ps_on_100000']] == fis[col['ps_on_100000']] == 1234.5
    assert g[lev[85000.0], col['ps_on_85000']] == fis[col['ps_on_85000']]
    assert np.isnan(g[lev[100000.0], col['ulp_below_100000']]) and np.isfinite(g[lev[92500.0], col['ulp_below_100000']])
    assert np.isfinite(g[lev[100000.0], col['ulp_above_100000']])
    assert np.isnan(g[:19, col['ps_2000']]).sum() == 9 and np.isnan(g[:, col['ps_nan']]).all()
    # the first five columns alone ascend: the single walk.  Same bits as in the general form above, tie level included
    five = [np.ascontiguousarray(e[k][..., :5]) for k in ('ps', 'fis', 'ta', 'hus')]
    walk = F.geopot_on_plev(five[0], five[1], five[2], five[3], e['ak'], e['bk'], e['plev'])
    assert np.array_equal(bits(walk), bits(got[..., :5]))
    # the tie level is half level k's pressure in every column: phi_hl[k] itself, whichever of the two layers that meet
    # there is taken (phi_hl[k + 1] + x and phi_hl[k + 1] - (-x) are one IEEE operation).  The level one ulp above it lies in
    # the layer below with a logarithm that differs by an ulp: continuous to rounding.  Alone in a list it gives the same bits
    p_tie, k = G.tie_level(e['ak'], e['bk'])
    beside = F.geopot_on_plev(five[0], five[1], five[2], five[3], e['ak'], e['bk'], [p_tie, np.nextafter(p_tie, np.inf)])
    np.testing.assert_allclose(beside[0, 0], beside[0, 1], rtol=1e-13)
    assert np.array_equal(bits(beside[0, 0]), bits(walk[0, lev[p_tie]]))


# ---- 2. two states -----------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def pgw_state(grid, nlev, seed, target):
    c = case(grid, nlev, seed, 'float64', target)
    w = O.pgw_for_era5_arrays(c['era'], c['deltas'], c['delta_times'], c['plev'], c['target_dt'], ignore_top_pressure_error=True)
    return w


STORAGE = {'f64/f64': ('float64', 'float64', 'float64'), 'f32 ERA + f64 PGW, f32 2-D': ('float32', 'float64', 'float32'),
           'f32/f32': ('float32', 'float32', 'float32')}


@pytest.mark.parametrize('instant', ['lerp', 'record'])
@pytest.mark.parametrize('storage', sorted(STORAGE))
@pytest.mark.parametrize('grid,nlev,seed', [((6, 11), 12, 3), ((15, 20), 21, 7)])
def test_two_states(F, grid, nlev, seed, storage, instant):
    from pgw4era5_amd import step_03_apply_to_era as s3
    target = dict(lerp=LERP, record=RECORD)[instant]
    c = case(grid, nlev, seed, 'float64', target)
    era, w = c['era'], pgw_state(grid, nlev, seed, target)
    ta_, tb_, t2_ = (np.dtype(x) for x in STORAGE[storage])
    a = (era['PS'].astype(t2_), era['T'].astype(ta_), era['QV'].astype(ta_))
    b = (w['PS'].astype(t2_), w['T'].astype(tb_), w['QV'].astype(tb_))
    fis, ak, bk, plev = era['FIS'].astype(t2_), era['ak'], era['bk'], c['plev']
    ib, ia, x_hi, x_new, keep = s3.delta_time_bracket(c['delta_times'], target)
    assert (x_hi == 0.0) == (instant == 'record')
    zb, za = c['deltas']['zg'][keep[ib]].astype(t2_), c['deltas']['zg'][keep[ia]].astype(t2_)
    want_change = G.phi_change(a, b, fis, ak, bk, plev)
    want_error = G.phi_error(a, b, fis, ak, bk, plev, zb, za, x_hi, x_new)
    scale = max(np.nanmax(np.abs(G.phi_on_plev(*((a[0], fis) + a[1:]), ak, bk, plev))), 1.0)
    phi_a = F.geopot_on_plev(a[0], fis, a[1], a[2], ak, bk, plev)
    phi_b = F.geopot_on_plev(b[0], fis, b[1], b[2], ak, bk, plev)
    dzg = (zb[None], za[None], x_hi, x_new)
    zgd = zb[None].astype(np.float64) if x_hi == 0.0 else F.time_lerp(zb[None].astype(np.float64), za[None].astype(np.float64), x_hi, x_new)
    for form in (0, 1):
        change, nan_c = F.geopot_change_on_plev(*a, *b, fis, ak, bk, plev, counts=True, form=form)
        error, nan_e = F.geopot_change_on_plev(*a, *b, fis, ak, bk, plev, dzg=dzg, counts=True, form=form)
        assert np.array_equal(np.isnan(change), np.isnan(want_change)) and np.array_equal(np.isnan(error), np.isnan(want_error))
        np.testing.assert_allclose(change, want_change, rtol=0.0, atol=RT * scale, equal_nan=True)
        np.testing.assert_allclose(error, want_error, rtol=0.0, atol=RT * scale, equal_nan=True)
        assert nan_c.tolist() == nan_e.tolist() == np.isnan(want_change).sum(axis=(0, 2, 3)).tolist()
        # the composed calls: two one-state launches and a subtraction (and the interpolated record times g)
        assert np.array_equal(bits(change), bits(phi_b - phi_a)), form
        assert np.array_equal(bits(error), bits((phi_b - phi_a) - zgd * O.CON_G)), form
    print('%s %s columns=%d: max|phi_change - statement| = %.3e (bound %.3e)'
          % (storage, instant, grid[0] * grid[1], np.nanmax(np.abs(change - want_change)), RT * scale))


def test_two_states_on_edge_columns(F):
    """The general form (a column that does not ascend, a NaN PS) with two states: state b = state a with every PS 30 Pa
    higher; against the statement and the composed calls."""
    e = G.edge_case()
    ps_b = e['ps'] + 30.0
    a, b = (e['ps'], e['ta'], e['hus']), (ps_b, e['ta'] + 1.5, e['hus'])
    want = G.phi_change(a, b, e['fis'], e['ak'], e['bk'], e['plev'])
    phi_a = F.geopot_on_plev(a[0], e['fis'], a[1], a[2], e['ak'], e['bk'], e['plev'])
    phi_b = F.geopot_on_plev(b[0], e['fis'], b[1], b[2], e['ak'], e['bk'], e['plev'])
    for form in (0, 1):
        got, nan = F.geopot_change_on_plev(*a, *b, e['fis'], e['ak'], e['bk'], e['plev'], counts=True, form=form)
        assert np.array_equal(bits(got), bits(phi_b - phi_a))
        assert np.array_equal(np.isnan(got), np.isnan(want))
        np.testing.assert_allclose(got, want, rtol=0.0, atol=RT * np.nanmax(np.abs(phi_a)), equal_nan=True)
        assert nan.tolist() == np.isnan(want).sum(axis=(0, 2, 3)).tolist()


# ---- 3. closure, end to end ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('grid', [(6, 11), (15, 20)])
def test_closure_float64(F, grid):
    """The check on what the GPU run itself produced: max|phi_error| at p_ref is the loop's last max_err."""
    from pgw4era5_amd import settings as S, step_03_apply_to_era as s3
    c = case(grid, 21, 5)
    era = c['era']
    w = s3.pgw_for_era5_arrays(era, c['deltas'], c['delta_times'], c['plev'], c['target_dt'], ignore_top_pressure_error=True)
    ib, ia, x_hi, x_new, keep = s3.delta_time_bracket(c['delta_times'], c['target_dt'])
    dzg = (c['deltas']['zg'][keep[ib]][None], c['deltas']['zg'][keep[ia]][None], x_hi, x_new)
    err = F.geopot_change_on_plev(era['PS'], era['T'], era['QV'], w['PS'], w['T'], w['QV'], era['FIS'], era['ak'], era['bk'],
                                  c['plev'], dzg=dzg)
    phi = F.geopot_on_plev(era['PS'], era['FIS'], era['T'], era['QV'], era['ak'], era['bk'], c['plev'])
    tol = RT * np.nanmax(np.abs(phi))
    k = list(c['plev']).index(float(S.p_ref_inp))
    at_ref = np.nanmax(np.abs(err[0, k]))
    last = w['max_err'][w['n_iter'] - 1]
    print('columns=%d: max|phi_error(p_ref)| = %.17g, loop %.17g, tol %.3e' % (grid[0] * grid[1], at_ref, last, tol))
    assert abs(at_ref - last) <= tol
    assert at_ref <= S.thresh_phi_ref_max_error + tol


def test_closure_float32_reference_mode(F):
    """A float32 file in reference-dtype mode (float64 T / QV beside float32 PS): the check against the statement fed the
    file's own values.  No threshold assertion: the loop rounded to float32, the check does not."""
    from pgw4era5_amd import step_03_apply_to_era as s3
    c = case((6, 11), 21, 5, 'float32')
    era = c['era']
    w = s3.pgw_for_era5_arrays(era, c['deltas'], c['delta_times'], c['plev'], c['target_dt'], ignore_top_pressure_error=True,
                               ref_dtype=True)
    assert w['T'].dtype == np.float64 and w['PS'].dtype == np.float32
    ib, ia, x_hi, x_new, keep = s3.delta_time_bracket(c['delta_times'], c['target_dt'])
    zb, za = c['deltas']['zg'][keep[ib]], c['deltas']['zg'][keep[ia]]
    a, b = (era['PS'], era['T'], era['QV']), (w['PS'], w['T'], w['QV'])
    got = F.geopot_change_on_plev(*a, *b, era['FIS'], era['ak'], era['bk'], c['plev'], dzg=(zb[None], za[None], x_hi, x_new))
    want = G.phi_error(a, b, era['FIS'], era['ak'], era['bk'], c['plev'], zb, za, x_hi, x_new)
    scale = np.nanmax(np.abs(G.phi_on_plev(era['PS'], era['FIS'], era['T'], era['QV'], era['ak'], era['bk'], c['plev'])))
    assert np.array_equal(np.isnan(got), np.isnan(want))
    np.testing.assert_allclose(got, want, rtol=0.0, atol=RT * scale, equal_nan=True)
    k = list(c['plev']).index(30000.0)
    print('float32 reference mode: max|phi_error(p_ref)| = %.6g, loop %.6g' % (np.nanmax(np.abs(got[0, k])), w['max_err'][w['n_iter'] - 1]))


# ---- 4. statistics ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('ncol', [1, 257, 1030, 20000])
def test_level_stats_against_numpy(F, ncol):
    rng = np.random.default_rng(ncol)
    x = rng.standard_normal((5, ncol)) * np.array([1.0, 1e3, 1e-3, 50.0, 1.0])[:, None]
    x[rng.random((5, ncol)) < 0.2] = np.nan
    x[3] = np.nan                                                  # a row without a valid element
    if ncol > 1:
        x[0, 0], x[0, -1] = 7.0, -9.0                              # both ends count
    s1, s2 = F.level_stats(x), F.level_stats(x)
    ok = ~np.isnan(x)
    n = ok.sum(axis=1)
    assert s1['count'].tolist() == n.tolist() and s1['count'][3] == 0
    z = np.where(ok, x, 0.0)
    eps = 2.0 ** -52
    assert np.all(np.abs(s1['sum'] - z.sum(axis=1)) <= n * eps * np.abs(z).sum(axis=1))
    assert np.all(np.abs(s1['sumsq'] - (z * z).sum(axis=1)) <= n * eps * (z * z).sum(axis=1))
    assert np.array_equal(s1['maxabs'], np.abs(z).max(axis=1))
    for k in s1:
        assert np.array_equal(s1[k], s2[k]) and (s1[k].dtype.kind == 'i' or np.array_equal(bits(s1[k]), bits(s2[k]))), k


# ---- 5. check_file and the command line -------------------------------------------------------------------------------------
def test_check_file_and_command_line(tmp_path, capsys):
    from pgw4era5_amd import check_geopot as C, ncio, settings as S, step_03_apply_to_era as s3
    era_dir, delta_dir, pgw_dir, chk_dir = (str(tmp_path / d) for d in ('era', 'deltas', 'pgw', 'chk'))
    steps = [dt.datetime(2006, 8, 2, 0), dt.datetime(2006, 8, 2, 3)]
    for i, t in enumerate(steps):
        c = synthetic.make_case(nlat=10, nlon=10, nlev=20, seed=0, target_dt=t)          # one set of deltas, two instants
        synthetic.write_case_files(c, era_dir, delta_dir)
    s3._cli(['-i', era_dir, '-o', pgw_dir, '-d', delta_dir, '-f', '2006080200', '-l', '2006080203', '-H', '3', '-t'])
    capsys.readouterr()
    tables = C._cli(['-i', era_dir, '-g', pgw_dir, '-d', delta_dir, '-o', chk_dir, '-f', '2006080200', '-l', '2006080203', '-H', '3'])
    text = capsys.readouterr().out
    assert len(tables) == 2 and text.count('<- p_ref') == 2 and text.count('<= thresh_phi_ref_max_error') == 2
    plev = synthetic.PLEV19
    for t, table in zip(steps, tables):
        name = S.era5_file_name_base.format(t)
        ds = ncio.open_dataset(os.path.join(chk_dir, 'zgcheck_' + name), decode_times=False)
        era = ncio.open_dataset(os.path.join(era_dir, name), decode_times=False)
        for v in ('phi_change', 'phi_delta', 'phi_error'):
            assert tuple(ds[v].dims) == ('time', 'plev', 'lat', 'lon') and ds[v].shape == (1, 19, 10, 10) and ds[v].dtype == np.float64
        np.testing.assert_array_equal(ds['plev'].values, plev)
        for d in ('time', 'lat', 'lon'):
            np.testing.assert_array_equal(ds[d].values, era[d].values)
        err, change, delta = (np.asarray(ds[v].values) for v in ('phi_error', 'phi_change', 'phi_delta'))
        assert np.array_equal(bits(err), bits(change - delta))
        assert not np.isnan(delta).any()
        e2 = err.reshape(19, 100)
        ok = ~np.isnan(e2)
        z = np.where(ok, e2, 0.0)
        n = ok.sum(axis=1)
        assert table['n_valid'].tolist() == n.tolist() and np.all(n > 0)
        np.testing.assert_array_equal(table['plev'], plev)
        np.testing.assert_allclose(table['mean'], z.sum(axis=1) / n, rtol=1e-12, atol=1e-12 * np.abs(z).max())
        np.testing.assert_allclose(table['rms'], np.sqrt((z * z).sum(axis=1) / n), rtol=1e-12)
        np.testing.assert_array_equal(table['max'], np.abs(z).max(axis=1))
        np.testing.assert_array_equal(table['max_m'], table['max'] / 9.80665)
        assert table['max'][list(plev).index(30000.0)] <= S.thresh_phi_ref_max_error
    # a PGW file of another grid
    other = synthetic.make_case(nlat=9, nlon=10, nlev=20, seed=0, target_dt=steps[0])
    bad = synthetic.write_case_files(other, str(tmp_path / 'other'), str(tmp_path / 'other_deltas'))
    name = S.era5_file_name_base.format(steps[0])
    with pytest.raises(ValueError, match='another grid'):
        C.check_file(os.path.join(era_dir, name), bad, delta_dir, steps[0], str(tmp_path / 'never.nc'))
    assert not os.path.exists(str(tmp_path / 'never.nc'))


# ---- 6. argument errors reach no kernel ------------------------------------------------------------------------------------
def test_argument_errors_launch_nothing(F):
    from pgw4era5_amd.device import default_context
    ctx = default_context()
    era = case((6, 11), 12, 3)['era']
    good = (era['PS'], era['FIS'], era['T'], era['QV'], era['ak'], era['bk'])
    ctx.profile(True)
    ctx.profile_reset()
    try:
        for plev in ([np.nan], [np.inf], [1e-4], [-1.0], [], np.ones((2, 2)), np.linspace(1e3, 1e5, 65)):
            with pytest.raises(ValueError):
                F.geopot_on_plev(*good, plev)
        with pytest.raises(ValueError):
            F.geopot_on_plev(era['PS'], era['FIS'], era['T'][:, :5], era['QV'][:, :5], era['ak'], era['bk'], [5e4])
        with pytest.raises(ValueError):
            F.geopot_on_plev(era['PS'][..., :3], era['FIS'], era['T'], era['QV'], era['ak'], era['bk'], [5e4])
        with pytest.raises(ValueError):
            F.geopot_change_on_plev(era['PS'], era['T'], era['QV'], era['PS'], era['T'][:, :5], era['QV'][:, :5], era['FIS'],
                                    era['ak'], era['bk'], [5e4])
        with pytest.raises(ValueError):
            F.geopot_change_on_plev(era['PS'], era['T'], era['QV'], era['PS'], era['T'], era['QV'], era['FIS'], era['ak'], era['bk'],
                                    [5e4, 3e4], dzg=np.zeros((1, 3, 6, 11)))
        assert ctx.profile_get('integ_geopot') == (0, 0.0)
        # the C entry refuses the same level lists by itself
        with pytest.raises(ValueError, match='must be finite and greater than 1e-4'):
            import ctypes as C
            from pgw4era5_amd import _lib
            p = (C.c_double * 1)(1e-4)
            d = {k: ctx.to_device(np.ascontiguousarray(era[k])) for k in ('PS', 'FIS', 'T', 'QV')}
            out = ctx.empty((1, 1, 6, 11), np.float64)
            ctx.set_levels(era['ak'], era['bk'])
            ctx._check(ctx.lib.pgw_geopot_on_plev(ctx.handle, _lib.PGW_F64, _lib.PGW_F64, 0, 1, 1, 66, p, d['FIS'].ptr, d['PS'].ptr,
                                                  d['T'].ptr, d['QV'].ptr, None, None, None, 0, None, None, 0.0, 0.0, 9.80665, 0,
                                                  out.ptr, None))
        assert ctx.profile_get('integ_geopot') == (0, 0.0)
        F.geopot_on_plev(*good, [5e4])
        assert ctx.profile_get('integ_geopot')[0] == 1                                       # one launch per call
        F.geopot_change_on_plev(era['PS'], era['T'], era['QV'], era['PS'], era['T'], era['QV'], era['FIS'], era['ak'], era['bk'],
                                [5e4, 3e4], dzg=np.zeros((1, 2, 6, 11)))
        assert ctx.profile_get('integ_geopot')[0] == 2
    finally:
        ctx.profile(False)
