"""GPU checks of step_01 (pgw4era5_amd/step_01_extract_deltas.py and its three C-ABI entries).

Fused model-level -> pressure-level kernel: against the oracle's interp_logp_4d on the 4-D pressure fields this file
builds in numpy (float64 inputs: the float64 oracle; float32 inputs: the reference-dtype oracle) at the project's
tolerance for that function (tests/test_hip_parity.py::test_interp_logp_4d_vs_oracle: the only inexact step is the
logarithm, <= 1 ulp from numpy's); bit for bit against the composed function-level call; exact hits and the column ends;
the float32 difference of the reference's dtype flow; the three dispatch forms of tests/test_hip_dispatch.py.
Magnus kernel: against the reference's own outputs (tests/golden/ref_step01_vectors.npz).  Level merge: bit for bit
against a numpy restatement.  Command line: end to end on synthetic NetCDF-3 files.

Test fields: the tolerance is relative to the RESULT, and the one inexact step (two logarithms, each <= 1 ulp of ~11.5,
i.e. <= 1.8e-15 absolute) enters 'linear' extrapolation as |w * dy| * 3.6e-15 / (x2 - x1) with w = (x - x1) / (x2 - x1).
With 95 levels the top two lie 0.05 apart in ln p and the list reaches 3 ln-units above them (w ~ 60): white noise
of 2 K per level would extrapolate to values that cross zero (|w * dy| ~ 200 K against a result near 0) - a question put
badly, not an error of either side.  The level noise therefore scales with the spacing in ln p (a gradient of a few K
per ln-unit, as in an atmosphere), which keeps every extrapolated value of the order of the field itself.

'off' cases: the target list is cut to the pressures inside EVERY column's source range (at least 3 must remain, so
the one-level list has no 'off' case); one extra case keeps a target below a mountain column's surface and must raise
the reference's text."""
import os

import numpy as np
import pytest

from oracle import pgw_oracle as O, pgw_oracle_refdtype as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden')
RTOL, ATOL = 1e-10, 1e-12            # test_interp_logp_4d_vs_oracle
MODES = ['off', 'linear', 'constant', 'nan']
S_LIST, N_LIST = [2, 3, 19, 47, 95], [1, 19, 99]
# (nlat, nlon) per S: one column, odd widths, even widths, several blocks with a partial last block
GRID_OF_S = {2: (1, 1), 3: (3, 5), 19: (4, 6), 47: (9, 31), 95: (7, 150)}
# every mode on every (S, N); 'off' needs at least 3 targets inside every column, which the one-level list cannot give
CASES = [(m, S, N) for m in MODES for S in S_LIST for N in N_LIST if not (m == 'off' and N == 1)]
OFF_TEXT = 'Extrapolation deactivated but data out of bounds.'


def target_list(N):
    from pgw4era5_amd.synthetic import PLEV19
    if N == 99:
        return np.sort(np.loadtxt(os.path.join(GOLDEN, 'CFday_target_p_MPI-ESM1-2-HR.dat')))
    if N == 19:
        return np.sort(np.asarray(PLEV19, dtype=np.float64))
    assert N == 1
    return np.array([50000.0])


def hybrid_coefficients(S, rng):
    """ap, b (pressure ASCENDING with the index, top first): b = 0 on the top third (pure-pressure levels), both monotone;
    ap + b * ps ascends strictly for every ps >= 5e4 Pa."""
    k = np.arange(S)
    eta = 0.02 + 0.98 * (k / (S - 1.0))**1.5
    if S > 3:
        eta[1:-1] += rng.uniform(-0.2, 0.2, S - 2) * np.minimum(np.diff(eta)[:-1], np.diff(eta)[1:])
    n_pure = max(1, S // 3)
    eta_c = eta[n_pure - 1]
    b = np.where(k < n_pure, 0.0, (np.maximum(eta - eta_c, 0.0) / (1.0 - eta_c))**1.2)
    ap = (eta - b) * 1.0e5
    ap[-1], b[-1] = 0.0, 1.0
    assert np.all(np.diff(b) >= 0) and np.all(b[:n_pure] == 0) and np.all(np.diff(ap[:n_pure]) > 0 if n_pure > 1 else True)
    for ps in (5.0e4, 1.05e5):
        assert np.all(np.diff(ap + b * ps) > 0)
    return ap, b, n_pure


def make_case(S, N, dtype, seed, nt=2, grid=None, wind=False):
    rng = np.random.default_rng(1000 * S + 10 * N + seed)
    nlat, nlon = grid or GRID_OF_S[S]
    ap, b, n_pure = hybrid_coefficients(S, rng)
    ps = rng.uniform(5.0e4, 1.05e5, (nt, nlat, nlon))
    ps.flat[0] = 5.0e4                                              # the highest mountain
    ps = ps.astype(dtype)
    eta = (ap + b * 1.0e5) / 1.0e5
    # temperature-like: a profile plus level noise that scales with the level spacing in ln p, so that the vertical gradient
    # dT / dln p stays a few K whatever S is (see the module docstring: conditioning of 'linear')
    lnp = np.log(ap + b * 1.0e5)
    dln = np.minimum(np.gradient(lnp), 1.0)
    var = (200.0 + 90.0 * eta[None, :, None, None] + 2.0 * dln[None, :, None, None] * rng.normal(0, 1.0, (nt, S, nlat, nlon))).astype(dtype)
    if wind:        # values of both signs and many magnitudes: differences of neighbours are NOT exact in float32
        var = (rng.normal(0, 10.0, (nt, S, nlat, nlon)) * rng.uniform(0.01, 3.0, (nt, S, nlat, nlon))).astype(dtype)
    source_P = ap[None, :, None, None] + b[None, :, None, None] * ps[:, None]          # :91, float64
    assert source_P.dtype == np.float64 and np.all(np.diff(source_P, axis=1) > 0)
    return dict(ap=ap, b=b, n_pure=n_pure, ps=ps, var=var, source_P=source_P, targ=target_list(N))


def cut_for_off(case):
    """Targets inside every column's source range."""
    sp, t = case['source_P'], case['targ']
    keep = t[(t > sp[:, 0].max()) & (t < sp[:, -1].min())]
    return keep


def oracle(case, targ, mode):
    var, sp = case['var'], case['source_P']
    tp = np.broadcast_to(targ[None, :, None, None], (var.shape[0], len(targ)) + var.shape[2:])
    mod = O if var.dtype == np.float64 else R
    return mod.interp_logp_4d(var, sp, np.ascontiguousarray(tp), mode)


@pytest.fixture(scope='module')
def ctx():
    from pgw4era5_amd.device import default_context
    return default_context()


@pytest.fixture(scope='module')
def s1():
    from pgw4era5_amd import step_01_extract_deltas
    return step_01_extract_deltas


# ------------------------------------------------------------------------------- 5. fused kernel against the oracle
@pytest.mark.parametrize('dtype', ['float64', 'float32'])
@pytest.mark.parametrize('mode,S,N', CASES)
def test_fused_kernel_vs_oracle(s1, mode, S, N, dtype):
    case = make_case(S, N, np.dtype(dtype), seed=1)
    targ = case['targ']
    if mode == 'off':
        targ = cut_for_off(case)
        assert len(targ) >= 3
    want = oracle(case, targ, mode)
    assert want.dtype == np.float64
    if mode == 'nan' and N > 1:
        assert np.isnan(want).any() and not np.isnan(want).all()
    for src_rev in (False, True):
        for out_rev in (False, True):
            sl = slice(None, None, -1) if src_rev else slice(None)
            got = s1.interp_to_plev(np.ascontiguousarray(case['var'][:, sl]), case['ps'], case['ap'][sl], case['b'][sl], targ,
                                    extrapolate=mode, lev_descending=src_rev, plev_descending=out_rev)
            assert got.dtype == np.float64 and got.shape == want.shape
            w = want[:, ::-1] if out_rev else want
            np.testing.assert_allclose(got, w, rtol=RTOL, atol=ATOL, equal_nan=True, err_msg='%s %s' % (src_rev, out_rev))
    # level order found from ap / b
    got = s1.interp_to_plev(np.ascontiguousarray(case['var'][:, ::-1]), case['ps'], case['ap'][::-1], case['b'][::-1], targ, extrapolate=mode)
    np.testing.assert_allclose(got, want[:, ::-1], rtol=RTOL, atol=ATOL, equal_nan=True)


@pytest.mark.parametrize('dtype', ['float64', 'float32'])
def test_off_raises_the_reference_text_with_the_smallest_column(s1, dtype):
    case = make_case(19, 19, np.dtype(dtype), seed=2, grid=(6, 10))
    inside = cut_for_off(case)
    sp = case['source_P']
    p_bad = 0.5 * (sp[:, -1].min() + np.sort(sp[:, -1].ravel())[1])          # below the highest mountain's surface only
    targ = np.sort(np.concatenate([inside, [p_bad]]))
    with pytest.raises(ValueError) as e:
        oracle(case, targ, 'off')
    assert str(e.value) == OFF_TEXT
    with pytest.raises(ValueError) as e:
        s1.interp_to_plev(case['var'], case['ps'], case['ap'], case['b'], targ, extrapolate='off')
    assert str(e.value) == OFF_TEXT
    flat = np.nonzero((sp[:, -1] < p_bad).ravel())[0]
    assert len(flat) == 1 and e.value.column == flat[0] == 0
    # the context computes afterwards
    got = s1.interp_to_plev(case['var'], case['ps'], case['ap'], case['b'], inside, extrapolate='off', plev_descending=False)
    np.testing.assert_allclose(got, oracle(case, inside, 'off'), rtol=RTOL, atol=ATOL)


def test_not_ascending_errors(s1):
    case = make_case(19, 19, np.dtype('float64'), seed=3)
    with pytest.raises(ValueError) as e:                           # levels given top-first but declared surface-first
        s1.interp_to_plev(case['var'], case['ps'], case['ap'], case['b'], case['targ'], lev_descending=True)
    assert str(e.value) == 'Source pressure values must be ascending!'


# ------------------------------------------------------------------------------- 6. the composed call, bit for bit
@pytest.mark.parametrize('mode,S,N', [c for c in CASES if (c[1], c[2]) in [(2, 19), (19, 99), (95, 99), (47, 1)]])
def test_fused_is_the_composed_call_bit_for_bit(s1, mode, S, N):
    from pgw4era5_amd import functions as F
    case = make_case(S, N, np.dtype('float64'), seed=4)
    targ = cut_for_off(case) if mode == 'off' else case['targ']
    var, sp = case['var'], case['source_P']
    tp = np.ascontiguousarray(np.broadcast_to(targ[None, :, None, None], (var.shape[0], len(targ)) + var.shape[2:]))
    composed = F.interp_logp_4d(var, sp, tp, mode)
    fused = s1.interp_to_plev(var, case['ps'], case['ap'], case['b'], targ, extrapolate=mode, plev_descending=False)
    assert fused.dtype == composed.dtype == np.float64
    assert np.array_equal(fused.view(np.uint64), composed.view(np.uint64))


# ------------------------------------------------------------------------------- 7. exact hits and the column ends
@pytest.mark.parametrize('dtype', ['float64', 'float32'])
@pytest.mark.parametrize('mode', MODES)
def test_exact_hit_and_column_ends(s1, mode, dtype):
    case = make_case(19, 19, np.dtype(dtype), seed=5)
    ap, var = case['ap'], case['var']
    k = case['n_pure'] - 2
    assert k >= 1 and case['b'][k] == 0
    inside = cut_for_off(case)
    targ = np.sort(np.concatenate([[ap[k]], inside]))             # ap[k] lies inside every column: 'off' raises nothing
    i = int(np.nonzero(targ == ap[k])[0][0])
    hit = s1.interp_to_plev(var, case['ps'], ap, case['b'], targ, extrapolate=mode, plev_descending=False)
    assert np.array_equal(hit[:, i], var[:, k].astype(np.float64))          # bit for bit (float32 -> float64 is exact)
    if mode in ('constant', 'nan'):
        ends = s1.interp_to_plev(var, case['ps'], ap, case['b'], [10.0, 2.0e5], extrapolate=mode, plev_descending=False)
        if mode == 'constant':
            assert np.array_equal(ends[:, 0], var[:, 0].astype(np.float64)) and np.array_equal(ends[:, 1], var[:, -1].astype(np.float64))
        else:
            assert np.isnan(ends).all()


# ------------------------------------------------------------------------------- 8. the float32 difference is taken
def test_f32_to_f64_takes_the_difference_in_float32(s1):
    # a wind-like field: float32 differences of temperature-like neighbours (within a factor 2 of each other) are exact
    case = make_case(47, 99, np.dtype('float32'), seed=6, wind=True)
    targ = case['targ']
    want_ref = oracle(case, targ, 'constant')                                             # reference dtype flow
    tp = np.ascontiguousarray(np.broadcast_to(targ[None, :, None, None], want_ref.shape))
    want_cast = O.interp_logp_4d(case['var'].astype(np.float64), case['source_P'], tp, 'constant')    # cast first
    differ = want_ref != want_cast
    assert differ.any()
    got = s1.interp_to_plev(case['var'], case['ps'], case['ap'], case['b'], targ, plev_descending=False)
    np.testing.assert_allclose(got, want_ref, rtol=RTOL, atol=ATOL)
    assert (got != want_cast).any()
    # where the two flows are further apart than the tolerance, the kernel is on the reference's side
    far = np.abs(want_ref - want_cast) > 4 * (ATOL + RTOL * np.abs(want_ref))
    assert far.any()
    assert np.all(np.abs(got[far] - want_ref[far]) < np.abs(got[far] - want_cast[far]))
    # float32 output: the same float64 values narrowed once
    got32 = s1.interp_to_plev(case['var'], case['ps'], case['ap'], case['b'], targ, plev_descending=False, out_dtype='float32')
    assert got32.dtype == np.float32
    f64 = s1.interp_to_plev(case['var'].astype(np.float64), case['ps'].astype(np.float64), case['ap'], case['b'], targ, plev_descending=False)
    assert np.array_equal(got32, f64.astype(np.float32))


# ------------------------------------------------------------------------------- 9. Magnus kernel against the golden vectors
def _magnus_on_golden(s1, tag):
    z = np.load(os.path.join(GOLDEN, 'ref_step01_vectors.npz'), allow_pickle=False)
    QV, P, T, RH = (z['%s_%s' % (tag, k)] for k in ('QV', 'P', 'T', 'RH'))
    got = np.empty_like(RH)
    for p in np.unique(P):                                         # the kernel takes P per level: one call per pressure
        m = P == p
        n = int(m.sum())
        r = s1.specific_to_relative_humidity(QV[m].reshape(1, 1, 1, n), np.array([p]), T[m].reshape(1, 1, 1, n))
        assert r.dtype == np.float64
        got[m] = r.reshape(n)
    return got, RH


def test_magnus_kernel_float64_vs_reference_outputs(s1):
    got, want = _magnus_on_golden(s1, 'f64')
    dev = np.max(np.abs(got - want) / np.abs(want))
    print('\nMagnus float64: largest relative deviation from the reference outputs %.3e' % dev)
    np.testing.assert_allclose(got, want, rtol=1e-13, atol=0)


def test_magnus_kernel_float32_vs_reference_outputs(s1):
    got, want = _magnus_on_golden(s1, 'f32')
    dev = np.max(np.abs(got - want) / np.abs(want))
    print('\nMagnus float32: largest relative deviation from the reference outputs %.3e = %.2f float32 ulp' % (dev, dev / 2.0**-23))
    assert dev <= 2.4e-7                                           # 2 float32 ulp


def test_magnus_levels_layout(s1):
    """(time, plev, column) layout: every level takes its own pressure."""
    rng = np.random.default_rng(7)
    plev = np.array([100000., 85000., 50000., 25000., 1000.])
    T = rng.uniform(190., 320., (3, 5, 4, 7))
    QV = rng.uniform(1e-6, 2e-2, T.shape)
    got = s1.specific_to_relative_humidity(QV, plev, T)
    want = 0.263 * plev[None, :, None, None] * QV * (np.exp(17.67 * (T - 273.15) / (T - 29.65)))**(-1)
    np.testing.assert_allclose(got, want, rtol=1e-13, atol=0)
    got4 = s1.specific_to_relative_humidity(QV, np.broadcast_to(plev[None, :, None, None], T.shape), T)
    assert np.array_equal(got, got4)


# ------------------------------------------------------------------------------- 10. level merge, bit for bit
def _emon_levels():
    from pgw4era5_amd.synthetic import PLEV19
    amon = np.asarray(PLEV19, dtype=np.float64)
    emon = [amon[0]]
    for lo, hi in zip(amon[:-1], amon[1:]):
        if lo > 10000.:
            emon += [lo + (hi - lo) / 3., lo + 2. * (hi - lo) / 3.]
        emon.append(hi)
    return np.array(emon), amon


def _merge_numpy(hur, emon, amon_hur, amon):
    """Emon_convert_hus_to_hur.py:82-122 restated on plain arrays."""
    out = hur.copy()
    for l, p in enumerate(emon):
        if p not in amon:
            d = amon - p
            ib = np.nanargmin(np.where(d > 0, amon, np.nan)); ia = np.nanargmax(np.where(d < 0, amon, np.nan))
            h = hur[:, l]
            ha, hb = hur[:, list(emon).index(amon[ia])], hur[:, list(emon).index(amon[ib])]
            with np.errstate(invalid='ignore', divide='ignore'):
                wa = 1 - np.abs(h - ha) / (np.abs(h - ha) + np.abs(h - hb))
                wb = 1 - np.abs(h - hb) / (np.abs(h - ha) + np.abs(h - hb))
                out[:, l] = amon_hur[:, ia] * wa + amon_hur[:, ib] * wb
        else:
            out[:, l] = amon_hur[:, list(amon).index(p)]
    return out


@pytest.mark.parametrize('amon_dtype', ['float32', 'float64'])
def test_hur_merge_levels_is_the_numpy_restatement_bit_for_bit(s1, amon_dtype):
    emon, amon = _emon_levels()
    rng = np.random.default_rng(8)
    nt, nlat, nlon = 3, 5, 9
    hur = np.clip(60 + 30 * np.sin(np.linspace(0, 5, len(emon)))[None, :, None, None] + rng.normal(0, 8, (nt, len(emon), nlat, nlon)), 0.5, 110)
    amon_hur = np.clip(55 + rng.normal(0, 15, (nt, len(amon), nlat, nlon)), 0.5, 110).astype(amon_dtype)
    l = int(np.nonzero(emon == emon[emon < 92500.].max())[0][0])  # a level that is interpolated
    assert emon[l] not in amon
    tabs = s1.merge_level_table(emon, amon)
    hur[1, [l, tabs[1][l], tabs[2][l]], 2, 3] = 42.0               # three equal values: 0 / 0
    want = _merge_numpy(hur, emon, amon_hur, amon)
    got = s1.merge_hur_levels(hur, emon, amon_hur, amon)
    assert got.dtype == want.dtype == np.float64
    assert np.isnan(want[1, l, 2, 3]) and np.isnan(want).sum() == 1
    # the same NaN positions (the sign of a NaN made by 0 / 0 is the machine's: set on x86, clear on the GPU) and the same
    # bits everywhere else
    assert np.array_equal(np.isnan(got), np.isnan(want))
    assert np.array_equal(np.where(np.isnan(got), 0.0, got).view(np.uint64), np.where(np.isnan(want), 0.0, want).view(np.uint64))
    for i, p in enumerate(emon):
        if tabs[0][i] >= 0:                                        # Amon's bits
            assert np.array_equal(got[:, i], amon_hur[:, tabs[0][i]].astype(np.float64))
        else:                                                      # a convex combination (weights sum to 1 within rounding)
            a, b = amon_hur[:, tabs[3][i]].astype(np.float64), amon_hur[:, tabs[4][i]].astype(np.float64)
            g = got[:, i]
            ok = np.isfinite(g)
            lo, hi = np.minimum(a, b), np.maximum(a, b)
            assert np.all(g[ok] >= lo[ok] - 1e-13 * np.abs(lo[ok])) and np.all(g[ok] <= hi[ok] + 1e-13 * np.abs(hi[ok]))


def test_merge_requires_equal_coordinates(s1):
    from pgw4era5_amd import ncio
    emon, amon = _emon_levels()
    lat, lon, t = np.arange(3.), np.arange(4.), np.arange(2.)
    hur = ncio.Field(np.full((2, len(emon), 3, 4), 50.), ('time', 'plev', 'lat', 'lon'), dict(time=t, plev=emon, lat=lat, lon=lon))
    am = ncio.Field(np.full((2, len(amon), 3, 4), 40., np.float32), ('time', 'plev', 'lat', 'lon'), dict(time=t, plev=amon, lat=lat + 0.5, lon=lon))
    with pytest.raises(ValueError):
        s1.merge_hur_levels(hur, None, am, None)
    am.coords['lat'] = lat
    out = s1.merge_hur_levels(hur, None, am, None)
    assert isinstance(out, ncio.Field) and out.dims == hur.dims and out.values.dtype == np.float64


# ------------------------------------------------------------------------------- 11. command line end to end
def _write_cfday(path, case, nrec, var_name='ta'):
    """A CFday-like NetCDF-3 file: levels stored surface-first, ap / b / ps beside the variable."""
    from pgw4era5_amd import ncio
    var, ps = case['var'][:, ::-1], case['ps']
    nt, S, nlat, nlon = var.shape
    assert nt == nrec
    co = dict(time=np.arange(nrec) + 0.5, lev=np.linspace(1, 0, S), lat=np.linspace(-10, 10, nlat), lon=np.linspace(0, 30, nlon))
    at = dict(time=dict(units='days since 1850-1-1 00:00:00', calendar='proleptic_gregorian', axis='T'),
              lat=dict(units='degrees_north', standard_name='latitude'), lon=dict(units='degrees_east', standard_name='longitude'),
              lev=dict(formula='p = ap + b*ps'))
    ds = ncio.Dataset(attrs=dict(variable_id=var_name, source_id='synthetic'), record_dim='time')
    for d in ('time', 'lev', 'lat', 'lon'):
        ds[d] = ncio.Field(co[d], (d,), {d: co[d]}, at[d])
    ds['ap'] = ncio.Field(case['ap'][::-1].copy(), ('lev',), dict(lev=co['lev']), dict(units='Pa'))
    ds['b'] = ncio.Field(case['b'][::-1].copy(), ('lev',), dict(lev=co['lev']), {})
    ds['ps'] = ncio.Field(ps, ('time', 'lat', 'lon'), {}, dict(units='Pa', standard_name='surface_air_pressure'))
    ds[var_name] = ncio.Field(np.ascontiguousarray(var), ('time', 'lev', 'lat', 'lon'), {},
                              dict(units='K', standard_name='air_temperature', long_name='Air Temperature', cell_methods='time: mean'))
    ncio.to_netcdf(ds, path)
    return co, at


@pytest.mark.parametrize('dtype', ['float32', 'float64'])
def test_command_line_interp_to_plev(s1, tmp_path, dtype):
    from pgw4era5_amd import ncio
    nrec = 7
    case = make_case(19, 99, np.dtype(dtype), seed=9, nt=nrec, grid=(5, 9))
    inp = str(tmp_path / 'ta_CFday_in.nc')
    co, at = _write_cfday(inp, case, nrec)
    plist = os.path.join(GOLDEN, 'CFday_target_p_MPI-ESM1-2-HR.dat')
    blobs = []
    for tag, extra in (('one', ['--max_records', '1']), ('three', ['--max_records', '3']), ('all', [])):
        out = str(tmp_path / ('{}_out_%s.nc' % tag))
        done = s1.main(['interp_to_plev', '-i', str(tmp_path / '{}_CFday_in.nc'), '-o', out, '-v', 'ta', '-p', plist] + extra)
        assert done == [out.replace('{}', 'ta')] and os.path.exists(done[0])
        blobs.append(open(done[0], 'rb').read())
    assert blobs[0] == blobs[1] == blobs[2]
    ds = ncio.open_dataset(done[0], decode_times=False)
    assert set(ds.variables) == {'time', 'plev', 'lat', 'lon', 'ta'}
    ta = ds['ta']
    assert ta.dims == ('time', 'plev', 'lat', 'lon') and ta.values.dtype == np.float64 and ta.shape == (nrec, 99, 5, 9)
    plev = ds['plev'].values
    assert np.all(np.diff(plev) < 0) and np.array_equal(plev[::-1], case['targ'])
    for d in ('time', 'lat', 'lon'):
        assert np.array_equal(ds[d].values, co[d]) and ds[d].attrs == at[d]
    assert ta.attrs == dict(units='K', standard_name='air_temperature', long_name='Air Temperature', cell_methods='time: mean')
    assert ds.record_dim == 'time'
    want = oracle(case, case['targ'], 'constant')[:, ::-1]
    np.testing.assert_allclose(ta.values, want, rtol=RTOL, atol=ATOL)


def test_command_line_hus_to_hur(s1, tmp_path):
    from pgw4era5_amd import ncio
    emon, amon = _emon_levels()
    rng = np.random.default_rng(10)
    nt, nlat, nlon = 2, 4, 6
    co = dict(time=np.arange(nt) + 15.0, lat=np.linspace(-5, 5, nlat), lon=np.linspace(0, 10, nlon))
    shp = (nt, len(emon), nlat, nlon)
    ta = (210 + 80 * (emon / 1e5)[None, :, None, None] + rng.normal(0, 2, shp)).astype(np.float32)
    hus = (1e-2 * (emon / 1e5)[None, :, None, None]**3 * rng.uniform(0.3, 1.0, shp)).astype(np.float32)
    amon_hur = rng.uniform(5, 95, (nt, len(amon), nlat, nlon)).astype(np.float32)

    def write(path, name, data, plev, attrs, gattrs):
        ds = ncio.Dataset(attrs=gattrs, record_dim='time')
        c = dict(co, plev=plev, time=co['time'][:data.shape[0]])
        for d in ('time', 'plev', 'lat', 'lon'):
            ds[d] = ncio.Field(c[d], (d,), {d: c[d]}, dict(axis=d[0].upper()))
        ds[name] = ncio.Field(data, ('time', 'plev', 'lat', 'lon'), c, attrs)
        ncio.to_netcdf(ds, path)
    paths = {k: str(tmp_path / (k + '.nc')) for k in ('hus', 'ta', 'amon', 'hur')}
    write(paths['hus'], 'hus', hus, emon, dict(standard_name='specific_humidity', long_name='Specific Humidity', units='1'), dict(variable_id='hus', table_id='Emon'))
    write(paths['ta'], 'ta', ta, emon, dict(standard_name='air_temperature', units='K'), dict(variable_id='ta'))
    write(paths['amon'], 'hur', amon_hur, amon, dict(standard_name='relative_humidity', units='%'), dict(variable_id='hur', table_id='Amon'))
    s1.main(['hus_to_hur', paths['hus'], paths['ta'], paths['hur'], '-a', paths['amon']])
    ds = ncio.open_dataset(paths['hur'], decode_times=False)
    assert 'hur' in ds and 'hus' not in ds and ds.attrs['variable_id'] == 'hur' and ds.attrs['table_id'] == 'Emon'
    hur = ds['hur']
    assert hur.dims == ('time', 'plev', 'lat', 'lon') and hur.values.dtype == np.float64 and np.array_equal(ds['plev'].values, emon)
    # Emon_convert_hus_to_hur.py:155-161 as written: long_name is renamed, standard_name is overwritten by the copy
    assert hur.attrs == dict(standard_name='specific_humidity', long_name='Relative Humidity', units='1')
    rh = s1.specific_to_relative_humidity(hus, emon, ta)
    assert np.array_equal(hur.values, _merge_numpy(rh, emon, amon_hur, amon), equal_nan=True)
    ta_short = str(tmp_path / 'ta_short.nc')
    write(ta_short, 'ta', ta[:1], emon, {}, {})
    with pytest.raises(ValueError):
        s1.main(['hus_to_hur', paths['hus'], ta_short, paths['hur'], '-a', paths['amon']])


# ------------------------------------------------------------------------------- 12. dispatch forms
def _misaligned(ctx, host):
    from pgw4era5_amd.device import DeviceArray
    host = np.ascontiguousarray(host)
    base = ctx.empty((host.size + 1,), host.dtype)
    d = DeviceArray(ctx, host.shape, host.dtype, ptr=base.ptr + host.dtype.itemsize, owner=base)
    assert d.ptr % 16 != 0
    return d.copy_from(host)


@pytest.mark.parametrize('dtype,out_dtype', [('float32', None), ('float64', None), ('float32', 'float32')])
@pytest.mark.parametrize('grid', [(4, 6), (3, 5), (35, 30), (37, 29)])
def test_dispatch_forms_give_the_same_bits(ctx, s1, grid, dtype, out_dtype):
    case = make_case(19, 99, np.dtype(dtype), seed=11, nt=3, grid=grid)
    args = (case['ap'], case['b'], case['targ'])
    ref = s1.interp_to_plev(case['var'], case['ps'], *args, extrapolate='linear', out_dtype=out_dtype)
    old = ctx.set_option('force_vec1', 1)
    try:
        vec1 = s1.interp_to_plev(case['var'], case['ps'], *args, extrapolate='linear', out_dtype=out_dtype)
    finally:
        ctx.set_option('force_vec1', old)
    old = ctx.set_option('force_off64', 1)
    try:
        off64 = s1.interp_to_plev(case['var'], case['ps'], *args, extrapolate='linear', out_dtype=out_dtype)
    finally:
        ctx.set_option('force_off64', old)
    mis = s1.interp_to_plev(_misaligned(ctx, case['var']), _misaligned(ctx, case['ps']), *args, extrapolate='linear', out_dtype=out_dtype).numpy()
    dev = s1.interp_to_plev(ctx.to_device(case['var']), ctx.to_device(case['ps']), *args, extrapolate='linear', out_dtype=out_dtype).numpy()
    u = np.uint64 if ref.dtype == np.float64 else np.uint32
    for other in (vec1, off64, mis, dev):
        assert other.dtype == ref.dtype and np.array_equal(other.view(u), ref.view(u))
    # every time slab of the three-step call is the one-step call on that slab
    one = s1.interp_to_plev(case['var'][1:2], case['ps'][1:2], *args, extrapolate='linear', out_dtype=out_dtype)
    assert np.array_equal(one.view(u), ref[1:2].view(u))


def test_profiler_times_the_new_kernels(ctx, s1):
    case = make_case(19, 19, np.dtype('float32'), seed=12)
    ctx.profile(True)
    try:
        ctx.profile_reset()
        s1.interp_to_plev(case['var'], case['ps'], case['ap'], case['b'], case['targ'])
        n, ms = ctx.profile_get('hybrid_to_plev')
        assert n == 1 and ms > 0
        assert ctx.profile_get('interp_logp')[0] == 0
    finally:
        ctx.profile(False)


def test_labelled_and_device_inputs_come_back_in_kind(ctx, s1):
    from pgw4era5_amd import ncio
    from pgw4era5_amd.device import DeviceArray
    case = make_case(19, 19, np.dtype('float32'), seed=13)
    nt, S, nlat, nlon = case['var'].shape
    co = dict(time=np.arange(nt) + 0.5, lev=np.arange(S, dtype=np.float64), lat=np.linspace(-3, 3, nlat), lon=np.linspace(0, 5, nlon))
    var = ncio.Field(case['var'], ('time', 'lev', 'lat', 'lon'), co, dict(units='K'), 'ta')
    ps = ncio.Field(case['ps'], ('time', 'lat', 'lon'), {k: co[k] for k in ('time', 'lat', 'lon')}, dict(units='Pa'), 'ps')
    plain = s1.interp_to_plev(case['var'], case['ps'], case['ap'], case['b'], case['targ'])
    out = s1.interp_to_plev(var, ps, case['ap'], case['b'], case['targ'])
    assert isinstance(out, ncio.Field) and out.dims == ('time', 'plev', 'lat', 'lon') and out.attrs == dict(units='K') and out.name == 'ta'
    assert np.array_equal(out.coords['plev'], case['targ'][::-1]) and 'lev' not in out.coords
    for d in ('time', 'lat', 'lon'):
        assert np.array_equal(out.coords[d], co[d])
    assert np.array_equal(out.values, plain, equal_nan=True)
    dev = s1.interp_to_plev(ctx.to_device(case['var']), ctx.to_device(case['ps']), case['ap'], case['b'], case['targ'])
    assert isinstance(dev, DeviceArray) and dev.dtype == np.float64 and np.array_equal(dev.numpy(), plain, equal_nan=True)
