"""replace_delta_sfc (reference functions.py:343-366) at its ties and under NaN levels below the ground.

The rule is one strict comparison of the HIST surface pressure against the delta file's pressure levels; it decides which
level moves to ps_hist, which levels take the surface delta and whether the column is an error.  The device code holds it
three times (pgw_kernels.h: `sfc_level()`, the text in `k_delta_pair`, the text in `k_delta_quad`).  Every test here uses one
input: synthetic.make_case(seed=81, nlev=27) with ps_hist written ON levels, one ulp beside them and above all of them,
in columns that sit next to each other in a vector group, on both sides of a wave boundary and at the end of the grid;
and the same case with ta / hur NaN at every level with plev >= ps_hist (what CMIP pressure-level files carry below the
ground, and what the `fill` part of the rule exists to keep out of the result).

CPU tests (unmarked): the data tell `>` from `>=`; all oracles return the clean case's bits on the NaN variant; the error
columns.  GPU tests: every copy of the rule against the oracle, the variants against each other, the NaN variant against
the clean case bit for bit, the function-level entry, and the errors."""
import datetime as dt
import functools

import numpy as np
import pytest

from oracle import pgw_oracle as O
from oracle import pgw_oracle_refdtype as R

SEED, NLEV = 81, 27
GRIDS = {'6x11': (6, 11),        # 66 columns: no multiple of the vector width (scalar columns), one wave + 2 lanes
         '8x12': (8, 12)}        # 96 columns: vector path, one and a half waves
INSTANTS = {'lerp': None,                                  # make_case's default instant: between two records
            'record': dt.datetime(2006, 3, 15, 12)}        # exactly a record: the LERP = false instantiations
MODES = ('f64', 'f32_fast', 'f32_reference')
DTYPE = dict(f64=np.float64, f32_fast=np.float32, f32_reference=np.float32)
REF_DTYPE = dict(f64=None, f32_fast=False, f32_reference=True)
FIELDS = ('PS', 'T', 'QV', 'U', 'V', 'RELHUM_pgw')

# pgw_set_option sets of the file path; reference-dtype mode exists in the quad kernel only (pgw_step03_file refuses
# ref_dtype = 1 with quad = 0), so the two pair-kernel sets run in the other two modes
OPTION_SETS = (('default', {}), ('fused_first=0', dict(fused_first=0)), ('quad=0', dict(quad=0)),
               ('quad=0,force_vec1=1', dict(quad=0, force_vec1=1)), ('full_column=1', dict(full_column=1)),
               ('force_off64=1', dict(force_off64=1)), ('multipass=0', dict(multipass=0)))
REINTERP = (('fixed', 30000.0, None), ('local', None, 'local'))      # (name, the oracles' p_ref, the package's p_ref)


def option_sets(mode):
    return [(n, o) for n, o in OPTION_SETS if not (mode == 'f32_reference' and o.get('quad') == 0)]


# ------------------------------------------------------------------ tolerances of the GPU comparisons, each with its source
# ('close', rtol, atol): assert_allclose;  ('scaled', bound): max |got - want| / max|want| of the level (over lat, lon) < bound
TOL = {
    # tests/test_hip_parity.py::test_whole_file_odd_shapes (RELHUM_pgw: ::test_whole_file_vs_oracle, the same mode)
    ('f64', False): dict(PS=('close', 1e-9, 1e-12), T=('close', 1e-9, 1e-12), U=('close', 1e-9, 1e-12), V=('close', 1e-9, 1e-12),
                         QV=('close', 1e-9, 1e-18), RELHUM_pgw=('close', 1e-9, 1e-12)),
    ('f32_fast', False): dict(PS=('close', 1e-6, 1e-12), T=('close', 1e-6, 1e-12), U=('close', 1e-6, 1e-5), V=('close', 1e-6, 1e-5),
                              QV=('close', 3e-6, 1e-18), RELHUM_pgw=('close', 1e-6, 1e-5)),
    # ::test_reference_dtype_mode_vs_refdtype_oracle.  RELHUM_pgw has no assert there: it is RELHUM of the ERA state - whose
    # only float32 node chain is e_sat(T), the chain QV's bound is about (numpy's expf against the device's, one or two
    # float32 ulp = 2.4e-7 of the value) - plus a float64 delta, so it takes QV's bound in QV's form
    ('f32_reference', False): dict(PS=('close', 1.3e-7, 0), T=('close', 1e-9, 1e-9), U=('close', 1e-9, 1e-9), V=('close', 1e-9, 1e-9),
                                   QV=('scaled', 6e-7), RELHUM_pgw=('scaled', 6e-7)),
    # ::test_reinterp_mode_vs_oracle.  RELHUM_pgw has no assert there; it is re-interpolated like T / U / V and of their
    # size (1e2), so it takes their bound; in reference-dtype mode the one-ulp pressure shift (6e-8) times its gradient
    # (RELHUM ~ p^3 above 200 hPa in the synthetic file: 1.8e-7 of the value) adds to the e_sat chain's 2.4e-7: QV's bound
    ('f64', True): dict(PS=('close', 1e-9, 0), T=('close', 1e-9, 1e-9), U=('close', 1e-9, 1e-9), V=('close', 1e-9, 1e-9),
                        QV=('scaled', 1e-9), RELHUM_pgw=('close', 1e-9, 1e-9)),
    ('f32_fast', True): dict(PS=('close', 2e-6, 0), T=('close', 2e-6, 1e-5), U=('close', 2e-6, 1e-5), V=('close', 2e-6, 1e-5),
                             QV=('scaled', 5e-6), RELHUM_pgw=('close', 2e-6, 1e-5)),
    ('f32_reference', True): dict(PS=('close', 2.5e-7, 0), T=('close', 6e-8, 0), U=('close', 0, 2e-5), V=('close', 0, 2e-5),
                                  QV=('scaled', 6e-7), RELHUM_pgw=('scaled', 6e-7)),
}


def loosest_T_tolerance(max_abs_T):
    """The largest |got - want| any GPU test below lets pass in T, in K."""
    return max(spec['T'][2] + spec['T'][1] * max_abs_T for spec in TOL.values())


# ------------------------------------------------------------------ the inputs (one builder)
def widen(x):
    """float32 arrays of a dict as float64 (the fast mode computes in float64 on the stored values)."""
    return {k: (np.asarray(v, dtype=np.float64) if isinstance(v, np.ndarray) and v.dtype == np.float32 else v) for k, v in x.items()}


def ps_hist_values(plev, dtype):
    """[(label, value in the storage type, is a tie)], `p` the levels ascending."""
    p = np.sort(np.asarray(plev)).astype(dtype)
    up, down = dtype(np.inf), dtype(0)
    return [('p[-1]', p[-1], True),                                   # tie with max(plev): the `else` branch, S-2 moves
            ('p[-2]', p[-2], True),
            ('nextafter(p[-1], +inf)', np.nextafter(p[-1], up), False),     # above every level: only the last level moves
            ('p[-3]', p[-3], True),
            ('nextafter(p[-2], 0)', np.nextafter(p[-2], down), False),      # one ulp below a level
            ('p[-4]', p[-4], True),
            ('103000', dtype(103000.0), False),
            ('p[-6]', p[-6], True),
            ('nextafter(p[0], +inf)', np.nextafter(p[0], up), False),       # level 0 moves, the whole column is the surface delta
            ('p[1]', p[1], True)]


def edge_columns(ncol):
    """Columns 0 and 1 share a vector group; 63 and 64 straddle the wave boundary; the last column of the grid."""
    return [0, 1, 7, 18, 29, 40, 51, 63, 64, ncol - 1]


@functools.lru_cache(maxsize=None)
def edge_case(grid, dtype_name, instant):
    """dict(c = make_case result, tie = deltas with ps_hist on the edges (all 12 records: the time interpolation of two equal
    records is the record), nan = the same with ta / hur NaN wherever plev >= ps_hist, cols = {column: (label, value, tie)}).
    Shared between tests: nobody writes into it."""
    from pgw4era5_amd import synthetic
    nlat, nlon = GRIDS[grid]
    dtype = np.dtype(dtype_name).type
    kw = {} if INSTANTS[instant] is None else dict(target_dt=INSTANTS[instant])
    c = synthetic.make_case(nlat=nlat, nlon=nlon, nlev=NLEV, seed=SEED, dtype=dtype, **kw)
    tie = {k: v.copy() for k, v in c['deltas'].items()}
    flat = tie['ps_hist'].reshape(12, -1)
    cols = {}
    for col, (label, value, is_tie) in zip(edge_columns(nlat * nlon), ps_hist_values(c['plev'], dtype)):
        flat[:, col] = value
        assert flat[0, col] == value and flat.dtype == dtype
        cols[col] = (label, value, is_tie)
    nan = {k: v.copy() for k, v in tie.items()}
    under = np.asarray(c['plev'], dtype=np.float64)[None, :, None, None] >= nan['ps_hist'][:, None].astype(np.float64)
    assert 0.03 < under.mean() < 0.2 and under.any(axis=(0, 1)).mean() > 0.3
    for v in ('ta', 'hur'):
        nan[v][under] = np.nan
    for d in (tie, nan):
        for v in d.values():
            v.setflags(write=False)
    return dict(c=c, tie=tie, nan=nan, cols=cols, ncol=nlat * nlon)


def oracle_run(mode, case, deltas, reinterp=None, vert_interp=None):
    """The expectation of one mode: float64 -> O; fast float32 -> O on the float32 values widened; reference-dtype float32
    -> R; reinterp = the oracles' p_ref (30000.0 or None) -> the `_reinterp` oracles."""
    c = case['c']
    tail = (c['delta_times'], c['plev'], c['target_dt'], True)
    if mode == 'f32_reference':
        if reinterp is None:
            return R.pgw_for_era5_arrays(c['era'], deltas, *tail)
        return R.pgw_for_era5_arrays_reinterp(c['era'], deltas, *tail, p_ref=reinterp[0])
    if reinterp is None:
        kw = {} if vert_interp is None else dict(vert_interp=vert_interp)
        return O.pgw_for_era5_arrays(widen(c['era']), widen(deltas), *tail, **kw)
    return O.pgw_for_era5_arrays_reinterp(widen(c['era']), widen(deltas), *tail, p_ref=reinterp[0])


@functools.lru_cache(maxsize=None)
def expected(mode, grid, instant, reinterp=None):
    """Oracle result on the tie case, computed once per (mode, grid, instant, path)."""
    case = edge_case(grid, np.dtype(DTYPE[mode]).name, instant)
    return oracle_run(mode, case, case['tie'], reinterp)


def same_bits(a, b, keys=('PS', 'T', 'QV', 'U', 'V', 'RELHUM_pgw')):
    return all(np.array_equal(a[k], b[k], equal_nan=True) for k in keys)


# ================================================================== CPU
@pytest.mark.parametrize('instant', list(INSTANTS))
@pytest.mark.parametrize('grid', list(GRIDS))
def test_the_data_tell_a_strict_comparison_from_a_weak_one(monkeypatch, grid, instant):
    """`>` written as `>=` in the column rule: in every tie column T moves by at least 50 times the loosest tolerance any
    GPU test below applies to T (seen: 0.074 K = 2.5e-4 of max|T| at the weakest column, the tie with max(plev); the loosest
    tolerance is 2e-6 of T + 1e-5 K = 5.9e-4 K, the fast float32 mode with i_reinterp), in every other column by exactly 0.  So a comparison flipped at a tie, in any copy of the rule, cannot pass
    test_every_copy_of_the_rule_vs_oracle."""
    case = edge_case(grid, 'float64', instant)
    want = expected('f64', grid, instant)

    def weak_rule(plev_asc, ps_hist, delta, delta_sfc):
        S, ncol = delta.shape
        P = np.repeat(np.asarray(plev_asc, dtype=np.float64)[:, None], ncol, axis=1)
        D = np.array(delta, dtype=np.float64, copy=True)
        gt = ps_hist[None, :] >= P                         # the slip
        assert gt.any(axis=0).all()
        k = S - 1 - np.argmax(gt[::-1], axis=0)
        D = np.where(np.arange(S)[:, None] >= k[None, :], delta_sfc[None, :], D)
        P[k, np.arange(ncol)] = ps_hist
        return P, D
    monkeypatch.setattr(O, 'replace_delta_sfc_columns', weak_rule)
    bad = oracle_run('f64', case, case['tie'])
    monkeypatch.undo()
    ncol = case['ncol']
    moved = np.abs(bad['T'] - want['T']).reshape(-1, ncol).max(axis=0)
    need = 50 * loosest_T_tolerance(np.abs(want['T']).max())
    ties = [col for col, (_, _, is_tie) in case['cols'].items() if is_tie]
    assert len(ties) == 6
    for col in ties:
        label, value, _ = case['cols'][col]
        print('column %d ps_hist = %s: max|dT| = %.3e K (needed %.3e)' % (col, label, moved[col], need))
        assert moved[col] >= need, (col, label, moved[col], need)
    others = np.delete(np.arange(ncol), ties)
    assert (moved[others] == 0).all()
    for k in ('PS', 'QV', 'RELHUM_pgw'):
        d = np.abs(bad[k] - want[k]).reshape(-1, ncol).max(axis=0)
        assert (d[others] == 0).all(), k


@pytest.mark.parametrize('instant', list(INSTANTS))
@pytest.mark.parametrize('dtype_name', ['float64', 'float32'])
@pytest.mark.parametrize('grid', list(GRIDS))
def test_the_oracles_agree_on_the_nan_variant(grid, dtype_name, instant):
    """NaN at every underground ta / hur level: all oracles - O and R whole-file, their `_reinterp` forms with the fixed and
    the local reference level, the per-column C loops - return the clean case's bits and pass count.  This is the
    expectation test_underground_nan_is_masked_bit_for_bit leans on."""
    from oracle import pgw_oracle_c as C
    case = edge_case(grid, dtype_name, instant)
    modes = ('f64',) if dtype_name == 'float64' else ('f32_fast', 'f32_reference')
    for mode in modes:
        for reinterp in (None,) + tuple((r[1],) for r in REINTERP):
            clean = expected(mode, grid, instant, reinterp)
            nan = oracle_run(mode, case, case['nan'], reinterp)
            assert nan['n_iter'] == clean['n_iter'], (mode, reinterp)
            assert same_bits(nan, clean), (mode, reinterp)
            assert np.isfinite(nan['T']).all() and np.isfinite(nan['QV']).all()
    mode = modes[0]
    clean = expected(mode, grid, instant)
    for deltas in (case['tie'], case['nan']):
        per_column = oracle_run(mode, case, deltas, vert_interp=C.vert_interp_delta)
        assert per_column['n_iter'] == clean['n_iter']
        assert same_bits(per_column, clean)


def error_inputs(case, col):
    """[(what, deltas)]: ps_hist == min(plev) and a NaN ps_hist in column `col` of the plain (tie-free) case."""
    out = []
    for what, value in (('ps_hist == p[0]', np.min(case['c']['plev'])), ('NaN ps_hist', np.nan)):
        d = {k: v.copy() for k, v in case['c']['deltas'].items()}
        d['ps_hist'].reshape(12, -1)[:, col] = value
        out.append((what, d))
    return out


ERROR_COLUMN = 64            # of 66: the first live lane of the partial wave


@pytest.mark.parametrize('mode', ['f64', 'f32_reference'])
def test_the_error_columns_in_the_oracles(mode):
    """ps_hist == p[0] is no `ps_hist < min(plev)` (functions.py:360), and nothing compares below a NaN: both reach np.max
    of an empty argwhere, the bare ValueError - in O and in R."""
    case = edge_case('6x11', np.dtype(DTYPE[mode]).name, 'lerp')
    for what, deltas in error_inputs(case, ERROR_COLUMN):
        with pytest.raises(ValueError) as e:
            oracle_run(mode, case, deltas)
        assert str(e.value) == '', what
        with pytest.raises(ValueError) as e:
            oracle_run(mode, case, deltas, reinterp=(30000.0,))
        assert str(e.value) == '', what


# ================================================================== GPU
@pytest.fixture(scope='module')
def gpu():
    from pgw4era5_amd import step_03_apply_to_era as s3
    from pgw4era5_amd.device import default_context
    return s3, default_context()


_GPU_RESULTS = {}


def gpu_run(gpu, mode, grid, instant, variant, opt_name='default', opts=None, reinterp=None):
    """One file through s3.pgw_for_era5_arrays under a set of context options (restored in any case); each combination
    runs once per session.  variant: 'tie' or 'nan'; reinterp: an entry of REINTERP or None."""
    key = (mode, grid, instant, variant, opt_name, reinterp and reinterp[0])
    if key not in _GPU_RESULTS:
        s3, ctx = gpu
        case = edge_case(grid, np.dtype(DTYPE[mode]).name, instant)
        c = case['c']
        kw = {} if reinterp is None else dict(i_reinterp=True, p_ref=reinterp[2])
        old = {k: ctx.set_option(k, v) for k, v in (opts or {}).items()}
        try:
            _GPU_RESULTS[key] = s3.pgw_for_era5_arrays(c['era'], case[variant], c['delta_times'], c['plev'], c['target_dt'], True,
                                                       ref_dtype=REF_DTYPE[mode], **kw)
        finally:
            for k, v in old.items():
                ctx.set_option(k, v)
    return _GPU_RESULTS[key]


def assert_fields(got, want, spec, case, where):
    """Tie and neighbour columns one by one first (a failure names the boundary), then the whole arrays."""
    ncol = case['ncol']
    assert got['n_iter'] == want['n_iter'], where
    for k in FIELDS:
        g, w = np.asarray(got[k], dtype=np.float64), np.asarray(want[k], dtype=np.float64)
        assert g.shape == w.shape, (k, where)
        kind = spec[k][0]
        if kind == 'scaled':
            err = np.abs(g - w) / np.nanmax(np.abs(w), axis=(2, 3), keepdims=True)
        for col, (label, value, _) in case['cols'].items():
            msg = '%s, %s: column %d, ps_hist = %s = %r' % (k, where, col, label, value)
            if kind == 'close':
                np.testing.assert_allclose(g.reshape(-1, ncol)[:, col], w.reshape(-1, ncol)[:, col], rtol=spec[k][1], atol=spec[k][2],
                                           err_msg=msg)
            else:
                assert err.reshape(-1, ncol)[:, col].max() < spec[k][1], msg
        if kind == 'close':
            np.testing.assert_allclose(g, w, rtol=spec[k][1], atol=spec[k][2], err_msg='%s, %s' % (k, where))
        else:
            assert err.max() < spec[k][1], '%s, %s' % (k, where)


@pytest.mark.gpu
@pytest.mark.parametrize('instant', list(INSTANTS))
@pytest.mark.parametrize('grid', list(GRIDS))
@pytest.mark.parametrize('mode', MODES)
def test_every_copy_of_the_rule_vs_oracle(gpu, mode, grid, instant):
    """The quad kernel (fused first pass or not, 32- and 64-bit offsets), the pair kernels (vector and scalar columns) and
    the loop variants behind them on the tie case against the oracle of the mode, at the tolerances of the existing
    whole-file tests of that mode (TOL)."""
    case = edge_case(grid, np.dtype(DTYPE[mode]).name, instant)
    want = expected(mode, grid, instant)
    for name, opts in option_sets(mode):
        got = gpu_run(gpu, mode, grid, instant, 'tie', name, opts)
        assert_fields(got, want, TOL[(mode, False)], case, '%s %s %s [%s]' % (mode, grid, instant, name))


@pytest.mark.gpu
@pytest.mark.parametrize('instant', list(INSTANTS))
@pytest.mark.parametrize('grid', list(GRIDS))
@pytest.mark.parametrize('mode', MODES)
def test_the_reinterp_copy_of_the_rule_vs_oracle(gpu, mode, grid, instant):
    """i_reinterp = 1 (k_reinterp_pair through sfc_level, in every pass on moved target levels), fixed and local reference
    level, against the `_reinterp` oracles."""
    case = edge_case(grid, np.dtype(DTYPE[mode]).name, instant)
    for reinterp in REINTERP:
        want = expected(mode, grid, instant, (reinterp[1],))
        got = gpu_run(gpu, mode, grid, instant, 'tie', reinterp=reinterp)
        assert_fields(got, want, TOL[(mode, True)], case, '%s %s %s i_reinterp p_ref %s' % (mode, grid, instant, reinterp[0]))


@pytest.mark.gpu
@pytest.mark.parametrize('instant', list(INSTANTS))
@pytest.mark.parametrize('grid', list(GRIDS))
@pytest.mark.parametrize('mode', ['f64', 'f32_fast'])
def test_variants_stay_bit_identical_on_ties(gpu, mode, grid, instant):
    """tests/test_hip_parity.py::test_kernel_variants_are_bit_identical on the tie case: the variants differ in scheduling
    and addressing, not in arithmetic - and not in the rule."""
    a = gpu_run(gpu, mode, grid, instant, 'tie')
    for name, opts in option_sets(mode)[1:]:
        b = gpu_run(gpu, mode, grid, instant, 'tie', name, opts)
        assert a['n_iter'] == b['n_iter'] and a['max_err'] == b['max_err'], name
        for k in ('PS', 'T', 'U', 'V'):
            np.testing.assert_array_equal(a[k], b[k], err_msg='%s [%s]' % (k, name))
        if mode == 'f32_fast':
            # the documented exception: the quad kernel writes the final QV of the pure-pressure levels from the fp64 vapour
            # pressure, the pair / full-column variants store it in the storage type first (one float32 rounding apart)
            np.testing.assert_allclose(a['QV'], b['QV'], rtol=2.5e-7, atol=0, err_msg='QV [%s]' % name)
        else:
            np.testing.assert_array_equal(a['QV'], b['QV'], err_msg='QV [%s]' % name)


@pytest.mark.gpu
@pytest.mark.parametrize('instant', list(INSTANTS))
@pytest.mark.parametrize('grid', list(GRIDS))
@pytest.mark.parametrize('mode', MODES)
def test_underground_nan_is_masked_bit_for_bit(gpu, mode, grid, instant):
    """The rule never uses a ta / hur value at a level with plev >= ps_hist: with NaN there, every selectable path returns
    the bits of the clean case.  No tolerance: a cache carry or a blend in place of a select would show as a NaN."""
    runs = [dict(opt_name=n, opts=o) for n, o in option_sets(mode)] + [dict(reinterp=r) for r in REINTERP]
    for kw in runs:
        where = '%s %s %s %s' % (mode, grid, instant, kw.get('opt_name') or 'i_reinterp p_ref ' + kw['reinterp'][0])
        clean = gpu_run(gpu, mode, grid, instant, 'tie', **kw)
        nan = gpu_run(gpu, mode, grid, instant, 'nan', **kw)
        assert np.isfinite(nan['T']).all() and np.isfinite(nan['QV']).all(), where
        assert nan['n_iter'] == clean['n_iter'] and nan['max_err'] == clean['max_err'], where
        for k in ('PS', 'T', 'QV'):
            np.testing.assert_array_equal(nan[k], clean[k], err_msg='%s, %s' % (k, where))


@pytest.mark.gpu
@pytest.mark.parametrize('dtype_name', ['float64', 'float32'])
@pytest.mark.parametrize('grid', list(GRIDS))
def test_vert_interp_delta_on_the_full_tie_list(grid, dtype_name):
    """The function-level entry (k_vert_interp_delta through sfc_level) on all ten edges and on the NaN variant, float64 and
    float32 deltas on float64 target pressures, at the tolerance of test_hip_parity.py::test_vert_interp_delta_vs_oracle."""
    from pgw4era5_amd import functions as F
    case = edge_case(grid, dtype_name, 'lerp')
    c, tie, nan = case['c'], case['tie'], case['nan']
    era = widen(c['era'])
    _, pa = O.hybrid_pressure(era['ak'], era['bk'], era['PS'])
    psh = tie['ps_hist'][3:4]
    for var, sfc in (('ta', 'tas'), ('hur', 'hurs')):
        want = O.vert_interp_delta(tie[var][3:4], c['plev'], pa, tie[sfc][3:4], psh, ignore_top_pressure_error=True)
        want_nan = O.vert_interp_delta(nan[var][3:4], c['plev'], pa, tie[sfc][3:4], psh, ignore_top_pressure_error=True)
        np.testing.assert_array_equal(want_nan, want)
        got = F.vert_interp_delta(tie[var][3:4], pa, tie[sfc][3:4], psh, ignore_top_pressure_error=True, plev=c['plev'])
        got_nan = F.vert_interp_delta(nan[var][3:4], pa, tie[sfc][3:4], psh, ignore_top_pressure_error=True, plev=c['plev'])
        assert got.dtype == np.float64
        ncol = case['ncol']
        for col, (label, value, _) in case['cols'].items():
            np.testing.assert_allclose(got.reshape(-1, ncol)[:, col], want.reshape(-1, ncol)[:, col], rtol=1e-10, atol=1e-13,
                                       err_msg='%s: column %d, ps_hist = %s = %r' % (var, col, label, value))
        np.testing.assert_allclose(got, want, rtol=1e-10, atol=1e-13, err_msg=var)
        np.testing.assert_allclose(got_nan, want, rtol=1e-10, atol=1e-13, err_msg=var + ' (NaN variant)')
        np.testing.assert_array_equal(got_nan, got, err_msg=var + ' (NaN variant against the clean case)')


@pytest.mark.gpu
@pytest.mark.parametrize('path', ['default', 'quad=0', 'i_reinterp'])
@pytest.mark.parametrize('mode', ['f64', 'f32_fast'])
def test_errors_at_the_boundary_in_every_path(gpu, mode, path):
    """ps_hist == p[0] and a NaN ps_hist in one column: status 15 of a healthy kernel, the reference's bare ValueError with
    the column attached - from the quad kernel's text, the pair kernel's text and sfc_level (i_reinterp)."""
    s3, ctx = gpu
    case = edge_case('6x11', np.dtype(DTYPE[mode]).name, 'lerp')
    c = case['c']
    opts = dict(quad=0) if path == 'quad=0' else {}
    kw = dict(i_reinterp=True) if path == 'i_reinterp' else {}
    for what, deltas in error_inputs(case, ERROR_COLUMN):
        old = {k: ctx.set_option(k, v) for k, v in opts.items()}
        try:
            with pytest.raises(ValueError) as e:
                s3.pgw_for_era5_arrays(c['era'], deltas, c['delta_times'], c['plev'], c['target_dt'], True,
                                       ref_dtype=REF_DTYPE[mode], **kw)
        finally:
            for k, v in old.items():
                ctx.set_option(k, v)
        assert str(e.value) == '' and e.value.column == ERROR_COLUMN, (what, path)
