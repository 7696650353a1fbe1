"""Whole-file cases whose ta / hur / ua / va deltas stand on more than 64 pressure levels, and cases whose zg delta stands
on a plev axis of its own, shared by tests/test_wide_plev_host.py, test_wide_plev_hip.py and test_zg_axis_hip.py.  A plain
module: no fixtures, no pytest hooks.

Axes, in file order (descending):
  S = 99           the reference's CFday target list (tests/golden/CFday_target_p_MPI-ESM1-2-HR.dat);
  S = 64, 65, 128  np.geomspace(101000, 120, S) with the entry nearest 30000 Pa set to 30000 (the fixed reference level);
  top=0.4          the same down to 0.4 Pa, above the synthetic model top of 0.5 Pa: the model-top check passes on it.
S = 64 is the last axis of the narrow table, 65 the first of the wide one.

`build(shape, S, dtype)` is synthetic.make_case on such an axis, with the shapes and seeds of local_pref_cases.  Treat every
array as read-only: the results are shared."""
import functools
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import local_pref_cases as L                                                          # noqa: E402
from oracle import pgw_oracle as O                                                   # noqa: E402
from oracle import pgw_oracle_refdtype as R                                          # noqa: E402
from pgw4era5_amd import synthetic                                                   # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
SHAPES = L.SHAPES
WIDE = (65, 99, 128)
P_REF = 30000.0
MODES = ('f64', 'f32_fast', 'f32_reference')
DTYPE = dict(f64='float64', f32_fast='float32', f32_reference='float32')


@functools.lru_cache(maxsize=None)
def axis(S, top=120.0):
    if S == 99 and top == 120.0:
        p = np.sort(np.loadtxt(os.path.join(GOLDEN, 'CFday_target_p_MPI-ESM1-2-HR.dat')))[::-1].copy()
    else:
        p = np.geomspace(101000.0, top, S)
        p[np.argmin(np.abs(p - P_REF))] = P_REF
    assert len(p) == S and np.all(np.diff(p) < 0) and np.sum(p == P_REF) == 1
    p.setflags(write=False)
    return p


@functools.lru_cache(maxsize=None)
def build(shape, S, dtype, top=120.0):
    nlat, nlon, nlev = shape
    return synthetic.make_case(nlat, nlon, nlev, seed=L.SEEDS[shape], dtype=np.dtype(dtype), plev=axis(S, top))


def as_f64(c):
    """(era, deltas) with every float32 array widened: what the float64 oracle takes for a float32 file in fast mode."""
    era = {k: (np.asarray(v, dtype=np.float64) if isinstance(v, np.ndarray) and v.dtype == np.float32 else v)
           for k, v in c['era'].items()}
    return era, {k: np.asarray(v, dtype=np.float64) for k, v in c['deltas'].items()}


@functools.lru_cache(maxsize=None)
def oracle_file(shape, S, mode, reinterp=False):
    """The oracle's whole-file result with the fixed reference level P_REF and the model-top check off, computed once:
    pgw_oracle on float64 copies for 'f64' / 'f32_fast', pgw_oracle_refdtype on the float32 arrays for 'f32_reference'."""
    c = build(shape, S, DTYPE[mode])
    tail = (c['delta_times'], c['plev'], c['target_dt'], True)
    if mode == 'f32_reference':
        f = R.pgw_for_era5_arrays_reinterp if reinterp else R.pgw_for_era5_arrays
        return f(c['era'], c['deltas'], *tail, p_ref=P_REF)
    era, d = as_f64(c)
    f = O.pgw_for_era5_arrays_reinterp if reinterp else O.pgw_for_era5_arrays
    return f(era, d, *tail, p_ref=P_REF)


def column_facts(c):
    """What the delta kernels meet on the columns of a case (float64 oracle pieces): per column the source level that moves
    to ps_hist (`ksfc`, ascending index; S - 1 where ps_hist > max(plev)), whether ps_hist lies above every level, and per
    target level the ascending index of the upper end of its bracket on the plain axis (`upper`: 0 below the axis, S above)."""
    era, d = as_f64(c)
    plev = np.asarray(c['plev'], dtype=np.float64)
    asc = plev[::-1]
    akm, bkm = O.full_level_coeffs(era['ak'], era['bk'])
    _, pa = O.hybrid_pressure(era['ak'], era['bk'], era['PS'], akm, bkm)
    psh = O.load_delta_values(d['ps_hist'], c['delta_times'], c['target_dt'])
    above = psh > asc.max()
    ksfc = np.where(above, len(asc) - 1, np.sum(psh[..., None] > asc, axis=-1) - 1)
    upper = np.searchsorted(asc, pa, side='left')
    return dict(ksfc=ksfc, ps_hist_above=above, upper=upper, ps_hist=psh)


# ---------------------------------------------------------------------------------------- zg on an axis of its own
ZG_SEED = 3


@functools.lru_cache(maxsize=None)
def zg_case(shape, dtype):
    """ta / hur / ua / va on the 99-level axis, zg on synthetic.PLEV19: deltas['zg'] and `plev_zg` from a second make_case
    with the same seed and shape, whose ERA fields are the same arrays bit for bit (checked)."""
    nlat, nlon, nlev = shape
    c = synthetic.make_case(nlat, nlon, nlev, seed=ZG_SEED, dtype=np.dtype(dtype), plev=axis(99))
    z = synthetic.make_case(nlat, nlon, nlev, seed=ZG_SEED, dtype=np.dtype(dtype))
    for k in ('PS', 'FIS', 'T', 'QV', 'U', 'V'):
        assert np.array_equal(c['era'][k], z['era'][k]), k
    assert np.array_equal(c['deltas']['ps_hist'], z['deltas']['ps_hist'])
    c['deltas'] = dict(c['deltas'], zg=z['deltas']['zg'])
    c['plev_zg'] = np.asarray(synthetic.PLEV19, dtype=np.float64)
    return c


@functools.lru_cache(maxsize=None)
def zg_oracle(shape, mode):
    """The oracle's loop with the per-column reference level on zg_case: ta_pgw / hur_pgw composed on the 99-level axis as
    local_pref_cases._inputs composes them (pgw_oracle on float64 copies; for 'f32_reference' pgw_oracle_refdtype's pieces
    on the float32 arrays), the loop fed with the zg delta and PLEV19.  -> dict(ps_pgw, hus_pgw, n_iter, max_err, p_ref, ta)."""
    c = zg_case(shape, DTYPE[mode])
    if mode == 'f32_reference':
        M, era, d = R, c['era'], c['deltas']
    else:
        M = O
        era, d = as_f64(c)
    akm, bkm = M.full_level_coeffs(era['ak'], era['bk'])
    _, pa = M.hybrid_pressure(era['ak'], era['bk'], era['PS'], akm, bkm)
    ld = lambda k: M.load_delta_values(d[k], c['delta_times'], c['target_dt'])
    ta = era['T'] + M.vert_interp_delta(ld('ta'), c['plev'], pa, ld('tas'), ld('ps_hist'), True)
    hur = M.specific_to_relative_humidity(era['QV'], pa, era['T']) + \
        M.vert_interp_delta(ld('hur'), c['plev'], pa, ld('hurs'), ld('ps_hist'), True)
    trace = []
    kw = dict(trace=trace) if M is O else {}
    res = M.adjust_ps_loop_local_pref(era['ak'], era['bk'], akm, bkm, era['PS'], era['FIS'], era['T'], era['QV'], ta, hur,
                                      ld('zg'), c['plev_zg'], **kw)
    return dict(res, ta=ta, trace=trace)


def padded(c, extra=(50.0, 20.0)):
    """A local_pref_cases case with zg on an axis of its own: the case's plev with `extra` levels appended, and zero
    records for them.  The first match in file order never reaches them (they lie below every other level's pressure and
    every level above them already satisfies the test wherever they would)."""
    zg = c['deltas']['zg']
    pad = np.zeros((zg.shape[0], len(extra)) + zg.shape[2:], dtype=zg.dtype)
    out = dict(c)
    out['deltas'] = dict(c['deltas'], zg=np.concatenate([zg, pad], axis=1))
    out['plev_zg'] = np.concatenate([np.asarray(c['plev'], dtype=np.float64), np.asarray(extra, dtype=np.float64)])
    return out
