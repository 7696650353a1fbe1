"""The numpy statement of the hydrostatic check (pgw4era5_amd/check_geopot.py), built from the oracle alone, and the edge
columns its tests share.  No test here (tests/test_geopot_check_host.py checks it on the CPU).

For one state and every level p:  ok = (fix(pa_hl) >= p).any(axis=1);  phi = O.integ_geopot(pa_hl, FIS, T, QV, level1,
p_ref = where(ok, p, fix(pa_hl).max(axis=1))), NaN where ~ok - a column without a half level at or below the level makes the
reference raise (functions.py:162-165), the statement masks it instead.  One addition to that: a column whose PS is not
finite has fix(pa_hl) = 1e-4 everywhere, and the oracle would find k* = 0 for the substitute p_ref and raise KeyError; such a
column (never ok, p > 1e-4) is given a finite stand-in PS for the call and masked like the others.

All arithmetic is float64 on the stored values (np.asarray(x, float64)), whatever the storage dtype."""
import numpy as np

from oracle import pgw_oracle as O
from pgw4era5_amd import synthetic

CON_G = O.CON_G


def fix(p):
    with np.errstate(invalid='ignore'):
        return np.where(p > 0, p, 0.0001)                                   # functions.py:135


def f64(x):
    return np.asarray(x, dtype=np.float64)


def phi_on_plev(ps, fis, ta, hus, ak, bk, plev):
    """(time, S, lat, lon) float64: integ_geopot at every level of `plev` (any order), NaN where no half level has
    p_hl >= p."""
    ps, fis, ta, hus = f64(ps), f64(fis), f64(ta), f64(hus)
    ak, bk = f64(ak), f64(bk)
    level1 = np.arange(1, len(ak) + 1)
    pa_hl = ak[None, :, None, None] + ps[:, None] * bk[None, :, None, None]
    fixed = fix(pa_hl)
    finite = np.isfinite(ps)
    ps_call = np.where(finite, ps, 101325.0)
    pa_call = ak[None, :, None, None] + ps_call[:, None] * bk[None, :, None, None]
    top = fix(pa_call).max(axis=1)
    out = np.empty((ps.shape[0], len(plev)) + ps.shape[1:], dtype=np.float64)
    for i, p in enumerate(np.asarray(plev, dtype=np.float64)):
        ok = (fixed >= p).any(axis=1)
        phi = O.integ_geopot(pa_call, fis, ta, hus, level1, np.where(ok, p, top))
        out[:, i] = np.where(ok, phi, np.nan)
    return out


def zg_delta(zb, za, x_hi, x_new):
    """load_delta's time interpolation of two records (functions.py:282-292) in float64 on the stored values."""
    zb = f64(zb)
    if x_hi == 0.0:
        return zb
    return (f64(za) - zb) / x_hi * x_new + zb


def phi_change(a, b, fis, ak, bk, plev):
    """phi_b - phi_a for states a, b = (ps, ta, hus)."""
    return phi_on_plev(b[0], fis, b[1], b[2], ak, bk, plev) - phi_on_plev(a[0], fis, a[1], a[2], ak, bk, plev)


def phi_error(a, b, fis, ak, bk, plev, zb, za, x_hi, x_new):
    """(phi_b - phi_a) - g * zg_delta (step_03:289, 298 on every level); zb / za (S, lat, lon) records in the order of plev."""
    return phi_change(a, b, fis, ak, bk, plev) - CON_G * zg_delta(zb, za, x_hi, x_new)[None]


def tie_level(ak, bk):
    """ak[k] of the lowest pure-pressure half level (the largest k with bk[k] == 0): the pressure of that half level in
    every column."""
    k = int(np.nonzero(np.asarray(bk) == 0.0)[0][-1])
    return float(ak[k]), k


# ---- edge columns ------------------------------------------------------------------------------------------------------
EDGE_NLEV = 12
EDGE_NAMES = ('ps_on_100000', 'ps_on_85000', 'ulp_below_100000', 'ulp_above_100000', 'plain', 'ps_2000', 'ps_nan')


def edge_case(dtype=np.float64, seed=5):
    """Seven columns (1, 7) on synthetic.hybrid_coefficients(12) from a make_case state, their PS replaced by the edge
    values (in the storage dtype, so 'one ulp' is an ulp of that dtype).  Returns dict(ps, fis, ta, hus, ak, bk, plev, names);
    plev is PLEV19 plus the tie level (20 levels)."""
    dt = np.dtype(dtype)
    case = synthetic.make_case(nlat=1, nlon=len(EDGE_NAMES), nlev=EDGE_NLEV, seed=seed, dtype=dt)
    era = case['era']
    one = dt.type(100000.0)
    ps = np.array(era['PS'], copy=True)
    ps[0, 0, :] = [one, dt.type(85000.0), np.nextafter(one, dt.type(0)), np.nextafter(one, dt.type(np.inf)), era['PS'][0, 0, 4],
                   dt.type(2000.0), dt.type(np.nan)]
    fis = np.array(era['FIS'], copy=True)
    fis[0, 0, 0] = dt.type(1234.5)                                          # a surface geopotential that is not zero
    p_tie, _ = tie_level(era['ak'], era['bk'])
    plev = np.concatenate([synthetic.PLEV19, [p_tie]])
    return dict(ps=ps, fis=fis, ta=era['T'], hus=era['QV'], ak=era['ak'], bk=era['bk'], plev=plev, names=EDGE_NAMES)
