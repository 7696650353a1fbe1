"""PGW_OPT_FUSED_FIRST ('fused_first'): the delta kernel walks every column from the surface up and, for float64 files,
runs the first two scans of the surface-pressure loop on the way (phi_ref of the ERA state and pass 1), so the loop kernel
starts at pass 2.  The option changes who computes, never what: with it on (default) and off, in one process, every output
has the same bits, the loop runs the same number of passes and records the same max|err| history, and an error reaches
Python with the same message and column.  float32 files keep the loop kernel's own first scans whatever the option says
(DESIGN.md section 4); their cases here pin that the option is harmless there."""
import datetime as dt

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FIELDS = ('PS', 'T', 'QV', 'U', 'V', 'RELHUM_pgw')
RECORD = dt.datetime(2006, 3, 15, 12)          # an instant that is a delta record: no time interpolation (LERP off)
PLEV34 = np.concatenate([np.array([100000., 97500, 95000, 92500, 90000, 87500, 85000, 82500, 80000, 77500, 75000,
                                   70000, 65000, 60000, 55000, 50000, 45000, 40000, 35000, 30000, 25000, 22500,
                                   20000, 17500, 15000, 12500, 10000]),
                         np.array([7000., 5000., 3000., 2000., 1000., 500., 100.])])
STORAGE = {'f64': (np.float64, False), 'f32': (np.float32, False), 'f32ref': (np.float32, True)}


def _case(nlat=8, nlon=12, nlev=27, seed=81, dtype=np.float64, **kw):
    from pgw4era5_amd import synthetic
    return synthetic.make_case(nlat=nlat, nlon=nlon, nlev=nlev, seed=seed, dtype=dtype, **kw)


def _run(c, ref_dtype=False, **kw):
    from pgw4era5_amd import step_03_apply_to_era as s3
    return s3.pgw_for_era5_arrays(c['era'], c['deltas'], c['delta_times'], c['plev'], c['target_dt'], True,
                                  ref_dtype=ref_dtype, **kw)


def _both(c, ref_dtype=False, opts=None, **kw):
    """The file with fused_first = 1 and = 0 (other options as given, the same for both); loop_guess is set before each
    run, because every file leaves its own pass count there."""
    from pgw4era5_amd.device import default_context
    ctx = default_context()
    opts = dict(opts or {})
    guess = opts.pop('loop_guess', None)
    old = {k: ctx.set_option(k, v) for k, v in opts.items()}
    old['fused_first'] = ctx.get_option('fused_first')
    res = []
    try:
        for fused in (1, 0):
            ctx.set_option('fused_first', fused)
            if guess is not None:
                ctx.set_option('loop_guess', guess)
            try:
                res.append(_run(c, ref_dtype, **kw))
            except ValueError as e:
                res.append(e)
    finally:
        for k, v in old.items():
            ctx.set_option(k, v)
    return res


def _same(a, b):
    assert not isinstance(a, Exception) and not isinstance(b, Exception), (a, b)
    assert a['n_iter'] == b['n_iter']
    np.testing.assert_array_equal(np.asarray(a['max_err']), np.asarray(b['max_err']))
    for k in FIELDS:
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)


def test_option_defaults_to_on():
    from pgw4era5_amd.device import default_context
    assert default_context().get_option('fused_first') == 1


@pytest.mark.parametrize('target', [None, RECORD], ids=['lerp', 'record'])
@pytest.mark.parametrize('storage', sorted(STORAGE))
def test_fused_and_unfused_have_the_same_bits(storage, target):
    """Every instantiation: float64, float32 fast, float32 reference-dtype storage; an instant between two records and one
    that is a record.  The orography of synthetic.make_case puts the surface between 1013 and about 540 hPa, so the
    surface insertion falls on several delta levels and the waves pass p_ref at different model levels."""
    dtype, ref = STORAGE[storage]
    c = _case(dtype=dtype, target_dt=target)
    assert c['era']['PS'].min() < 70000.0 < c['era']['PS'].max()
    a, b = _both(c, ref)
    _same(a, b)


@pytest.mark.parametrize('storage', sorted(STORAGE))
def test_34_delta_levels(storage):
    dtype, ref = STORAGE[storage]
    c = _case(6, 10, 40, seed=61, dtype=dtype, plev=PLEV34)
    a, b = _both(c, ref)
    _same(a, b)


@pytest.mark.parametrize('opts', [dict(loop_guess=1), dict(loop_guess=2), dict(loop_guess=5), dict(loop_guess=8),
                                  dict(force_off64=1)], ids=lambda o: '-'.join('%s%d' % kv for kv in o.items()))
@pytest.mark.parametrize('storage', sorted(STORAGE))
def test_first_launch_lengths_and_64_bit_offsets(storage, opts):
    """A first loop launch of 1, 2, 5 or 8 passes (the file needs 6: continuation launches and speculated passes), and the
    64-bit byte-offset instantiation of the delta kernel."""
    dtype, ref = STORAGE[storage]
    c = _case(dtype=dtype)
    a, b = _both(c, ref, opts)
    _same(a, b)
    assert a['passes_launched'] == b['passes_launched']


@pytest.mark.parametrize('storage', sorted(STORAGE))
def test_several_blocks_and_a_partial_last_wave(storage):
    """23 x 29 = 667 columns: six blocks of the delta kernel, the last wave with 27 of 64 lanes."""
    dtype, ref = STORAGE[storage]
    c = _case(23, 29, 31, seed=5, dtype=dtype)
    a, b = _both(c, ref)
    _same(a, b)


def _bend_one_layer(c, ps_turn):
    """Alter ak at one half level so that the layer above it has zero thickness at ps = ps_turn and a negative one below:
    ps_mono_min (the smallest ps with strictly ascending half-level pressures) becomes ps_turn."""
    era = dict(c['era'])
    ak, bk = era['ak'].copy(), era['bk'].copy()
    l = len(ak) - 6
    assert bk[l + 1] > bk[l]
    ak[l + 1] = ak[l] - ps_turn * (bk[l + 1] - bk[l])
    era['ak'] = ak
    era['akm'] = 0.5 * (ak[1:] - ak[:-1]) + ak[:-1]
    era['bkm'] = 0.5 * (bk[1:] - bk[:-1]) + bk[:-1]
    return dict(c, era=era)


@pytest.mark.parametrize('storage', ['f64', 'f32'])
def test_groups_without_ascending_pressures_next_to_groups_with(storage):
    """ps_mono_min inside the file's range of surface pressures: waves of the delta kernel that hold a column below it leave
    the ERA-state scan to the loop kernel, their neighbours do not; the file is the same as without the fusion and, in
    float64, the oracle's."""
    from oracle import pgw_oracle as O
    dtype, ref = STORAGE[storage]
    c = _bend_one_layer(_case(23, 29, 31, seed=5, dtype=dtype), 75000.0)
    ps = c['era']['PS'].reshape(-1)
    low = np.array([(ps[i:i + 64] < 75000.0).any() for i in range(0, ps.size, 64)])
    assert low.any() and not low.all()                 # groups of 64 columns of both kinds
    a, b = _both(c, ref)
    _same(a, b)
    if storage == 'f64':
        want = O.pgw_for_era5_arrays(c['era'], c['deltas'], c['delta_times'], c['plev'], c['target_dt'], True)
        assert a['n_iter'] == want['n_iter']
        for k in ('PS', 'T', 'QV', 'U', 'V'):
            np.testing.assert_allclose(a[k], want[k], rtol=1e-9, atol=1e-12, err_msg=k)


def _same_error(a, b):
    assert isinstance(a, ValueError) and isinstance(b, ValueError), (a, b)
    assert str(a) == str(b)
    assert getattr(a, 'column', None) == getattr(b, 'column', None)


@pytest.mark.parametrize('storage', sorted(STORAGE))
def test_nan_surface_pressure_in_a_few_columns(storage):
    """NaN PS in columns of the second and fifth group of 64: those groups are left to the loop kernel, the file ends as
    it does without the fusion (the reference raises on the all-NaN column)."""
    from oracle import pgw_oracle as O
    dtype, ref = STORAGE[storage]
    c = _case(23, 29, 31, seed=5, dtype=dtype)
    era = dict(c['era'])
    era['PS'] = c['era']['PS'].copy()
    for col in (70, 71, 300):
        era['PS'][0, col // 29, col % 29] = np.nan
    c = dict(c, era=era)
    a, b = _both(c, ref)
    _same_error(a, b)
    with pytest.raises(ValueError):
        O.pgw_for_era5_arrays(c['era'], c['deltas'], c['delta_times'], c['plev'], c['target_dt'], True)


@pytest.mark.parametrize('storage', sorted(STORAGE))
def test_p_ref_below_the_surface_is_reported_alike(storage):
    """Error 13 found by the delta kernel's scan: same message, same column as from the loop kernel's."""
    dtype, ref = STORAGE[storage]
    c = _case(23, 29, 31, seed=5, dtype=dtype)
    era = dict(c['era'])
    era['PS'] = c['era']['PS'].copy()
    era['PS'][0, 17, 5] = 20000.0                      # p_ref = 300 hPa lies below this "surface"
    c = dict(c, era=era)
    a, b = _both(c, ref)
    _same_error(a, b)
    assert 'p_ref locally lies below the surface' in str(a) and a.column == 17 * 29 + 5


def test_two_latitude_bands_give_the_unfused_one_rank_bits(tmp_path):
    """The two-band split of tests/test_hip_files.py (reduce hook, fused path in both bands) against ONE rank without the
    fusion."""
    from test_hip_files import _run_bands
    from pgw4era5_amd import synthetic
    from pgw4era5_amd.device import default_context
    msgs = _run_bands(tmp_path, 'clean', port='29561')
    assert msgs == {0: 'ok', 1: 'ok'}
    case = synthetic.make_case(nlat=21, nlon=32, nlev=40, seed=11, dtype=np.float64)
    ctx = default_context()
    old = ctx.set_option('fused_first', 0)
    try:
        whole = _run(case)
    finally:
        ctx.set_option('fused_first', old)
    bands = [np.load(str(tmp_path / ('band%d.npz' % r))) for r in range(2)]
    for b in bands:
        assert int(b['n_iter']) == whole['n_iter']
        np.testing.assert_array_equal(b['max_err'], np.asarray(whole['max_err']))
    for k in ('PS', 'T', 'QV', 'U', 'V'):
        np.testing.assert_array_equal(np.concatenate([bands[0][k], bands[1][k]], axis=-2), whole[k], err_msg=k)
