"""Cases and the numpy statement of the delta check (pgw4era5_amd/check_deltas.py, `pgw_state_on_plev`): host code only.

The statement is the definition put together from the oracle's restatements of the reference: pa = akm + PS * bkm
(`hybrid_pressure`), RH = `specific_to_relative_humidity(QV, pa, T)`, X(p) = `interp_logp_4d(X, pa, p, 'nan')` for X in
(T, RH, U, V), delta and ps_hist through `load_delta_values`, all on float64-widened inputs.  A column with pa[N-1] < pa[0]
is NaN on every level (the oracle's interp_logp_4d raises for it; the statement masks it).

`conditions()` asserts on the CPU what the cases exist for (tests/test_delta_check_host.py calls it)."""
import functools

import numpy as np

from oracle import pgw_oracle as O
from pgw4era5_amd import synthetic

VARS = ('ta', 'hur', 'ua', 'va')
PLEV19 = synthetic.PLEV19
PLEV5 = np.array([100000.0, 70000.0, 30000.0, 10000.0, 1000.0])
GRIDS = {1: (1, 1), 66: (6, 11), 96: (8, 12), 300: (15, 20)}        # one column; a wave + 2; a wave and a half; two blocks, ragged
NLEVS = (2, 12, 21)
SEED = 11
MIN_DISTANCE = 1e-9                                                  # relative: no bracket hangs on the last bit of a logarithm


def level_list(S):
    """S levels of PLEV19 spread over the axis (S = 1: 50000 Pa), in the file's descending order."""
    if S == 1:
        return np.array([50000.0])
    return np.ascontiguousarray(PLEV19[np.unique(np.round(np.linspace(0, 18, S)).astype(int))])


# ------------------------------------------------------------------ the statement
def _f64(x):
    return np.asarray(x, dtype=np.float64)


def state_on_plev(ps, ta, hus, ua, va, ak, bk, plev):
    """(4, time, S, H0, H1) float64: T, RH, U, V on the levels `plev` (any order, repeats allowed)."""
    ps, ta, hus, ua, va = (_f64(x) for x in (ps, ta, hus, ua, va))
    plev = _f64(plev)
    with np.errstate(all='ignore'):
        pa = O.hybrid_pressure(ak, bk, ps)[1]
        rh = O.specific_to_relative_humidity(hus, pa, ta)
        bad = pa[:, -1] < pa[:, 0]                                     # (time, H0, H1); False for a NaN PS
        pa_use = np.where(bad[:, None], O.hybrid_pressure(ak, bk, np.full_like(ps, 1.0e5))[1], pa)
        order = np.argsort(plev, kind='stable')
        targ = np.broadcast_to(plev[order][None, :, None, None], (ps.shape[0], plev.size) + ps.shape[1:]).copy()
        out = np.empty((4,) + targ.shape)
        for i, x in enumerate((ta, rh, ua, va)):
            out[i][:, order] = O.interp_logp_4d(x, pa_use, targ, 'nan')
        out[:, np.broadcast_to(bad[:, None], targ.shape)] = np.nan
    return out


def state_change(a, b, ak, bk, plev):
    """X_b - X_a; a, b = (ps, ta, hus, ua, va)."""
    return state_on_plev(*b, ak, bk, plev) - state_on_plev(*a, ak, bk, plev)


def delta_at(values, delta_times, target):
    """The delta of one variable at the instant: load_delta on its own time axis, (1, ...) float64."""
    return O.load_delta_values(_f64(values), delta_times, target)


def state_error(a, b, ak, bk, plev, deltas, times_by_var, target):
    """change - delta where plev < ps_hist, NaN elsewhere; `deltas`: dict of record arrays (nrec, S, H0, H1) for ta, hur, ua,
    va in the order of `plev`, and (nrec, H0, H1) for ps_hist; `times_by_var`: the time axis of each."""
    change = state_change(a, b, ak, bk, plev)
    psh = delta_at(deltas['ps_hist'], times_by_var['ps_hist'], target)                       # (1, H0, H1)
    with np.errstate(invalid='ignore'):
        above = _f64(plev)[None, :, None, None] < psh[:, None]
    err = np.full_like(change, np.nan)
    for i, v in enumerate(VARS):
        d = delta_at(deltas[v], times_by_var[v], target)
        err[i] = np.where(above, change[i] - d, np.nan)
    return err


# ------------------------------------------------------------------ the kernel cases
def smooth(shape3):
    """A smooth field in [0, 1] over (time, H0, H1)."""
    j, i = np.meshgrid(np.arange(shape3[1]), np.arange(shape3[2]), indexing='ij')
    return np.broadcast_to(0.5 * (1.0 + np.sin(0.7 * i + 0.3) * np.cos(0.4 * j)), shape3).copy()


def state_b_of(era):
    """State b of the kernel cases, made on the host: PS_a + a smooth 50 - 300 Pa, the fields + smooth offsets."""
    s = smooth(era['PS'].shape)
    s4 = s[:, None]
    dt = era['T'].dtype
    return dict(PS=(era['PS'] + (50.0 + 250.0 * s)).astype(era['PS'].dtype), T=(era['T'] + (1.5 + s4)).astype(dt),
                QV=(era['QV'] * (1.0 + 0.05 * s4)).astype(dt), U=(era['U'] + (0.8 * s4 - 0.3)).astype(dt),
                V=(era['V'] + (0.2 - 0.5 * s4)).astype(dt))


def fields(state):
    return state['PS'], state['T'], state['QV'], state['U'], state['V']


@functools.lru_cache(maxsize=None)
def case(ncol, nlev, dtype='float64', target=None, plev5=False):
    """synthetic.make_case on the grid of `ncol` columns, with state b; read-only arrays."""
    nlat, nlon = GRIDS[ncol] if ncol in GRIDS else ncol
    c = synthetic.make_case(nlat=nlat, nlon=nlon, nlev=nlev, seed=SEED, dtype=np.dtype(dtype), target_dt=target,
                            plev=PLEV5 if plev5 else None)
    c['b'] = state_b_of(c['era'])
    for d in (c['era'], c['b'], c['deltas']):
        for v in d.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
    return c


def shifted_axes(delta_times):
    """Five different time axes: the stamps of variable i moved by 2 i days."""
    t = np.asarray(delta_times).astype('datetime64[s]')
    return {v: t + np.timedelta64(2 * i, 'D') for i, v in enumerate(VARS + ('ps_hist',))}


# ------------------------------------------------------------------ the edge columns
# half levels chosen so that the full-level coefficients are exact: (9000 + 11000) / 2 = 10000, a pure-pressure full level
EDGE_AK = np.array([0.0, 2000.0, 9000.0, 11000.0, 8000.0, 3000.0, 0.0])
EDGE_BK = np.array([0.0, 0.0, 0.0, 0.0, 0.3, 0.7, 1.0])
# a hybrid top level: its pressure moves with PS, so a level can lie above the top full level in one state only
TOP_AK = np.array([0.0, 780.0, 9000.0, 11000.0, 8000.0, 3000.0, 0.0])
TOP_BK = np.array([0.0, 0.002, 0.002, 0.01, 0.3, 0.7, 1.0])
EDGE_NAMES = ('plain', 'low_in_a', 'psh_on_level', 'psh_ulp_above', 'psh_ulp_below', 'psh_nan', 'ps_nan', 't_nan', 'wind_sign',
              'descending', 'plain2')


def edge_case(ncol=None, dtype=np.float64, hybrid_top=False):
    """Columns (1, N, 1, ncol) that carry one property each, two states and records for them.  `ncol` > the number of edge
    columns: they stand at the start (neighbouring each other) and again at the end (the last column is one of them), plain
    columns between.  dict ak, bk, plev, a, b (ps, ta, hus, ua, va), deltas, times, target, names (column -> name)."""
    ak, bk = (TOP_AK, TOP_BK) if hybrid_top else (EDGE_AK, EDGE_BK)
    ne = len(EDGE_NAMES)
    ncol = ne if ncol is None else ncol
    assert ncol >= ne and (ncol == ne or ncol >= 2 * ne)
    names = list(EDGE_NAMES) + ['plain'] * (ncol - 2 * ne) + (list(EDGE_NAMES) if ncol > ne else [])
    n, N = len(names), len(ak) - 1
    col = np.arange(n)
    k = np.arange(N)[:, None]
    ps_a = 100000.0 + 37.0 * (col % 5)
    ps_b = ps_a + 120.0 + 11.0 * (col % 3)
    ta = 215.0 + 11.0 * k + 0.25 * (col % 7)[None, :]
    hus = 1e-5 * (1.0 + k) ** 2.5 * (1.0 + 0.01 * (col % 4))[None, :]
    ua = 20.0 - 3.0 * k + 0.5 * (col % 6)[None, :]
    va = -4.0 + 1.5 * k - 0.25 * (col % 5)[None, :]
    a = dict(PS=ps_a.copy(), T=ta.copy(), QV=hus.copy(), U=ua.copy(), V=va.copy())
    b = dict(PS=ps_b.copy(), T=ta + 2.0, QV=hus * 1.04, U=ua + 0.7, V=va - 0.4)
    psh = np.full(n, 101000.0)
    for i, name in enumerate(names):
        if name == 'low_in_a':                  # the lowest full level of state a alone lies above 85000 Pa (EDGE: 82250 Pa)
            a['PS'][i], b['PS'][i] = 95000.0, 100000.0
            if hybrid_top:                      # ... and its top full level alone below 500 Pa: 390 + 0.001 PS = 485 / 510 Pa
                a['PS'][i], b['PS'][i] = 95000.0, 120000.0
        elif name == 'psh_on_level':
            psh[i] = 50000.0
        elif name == 'psh_ulp_above':
            psh[i] = np.nextafter(50000.0, np.inf)
        elif name == 'psh_ulp_below':
            psh[i] = np.nextafter(50000.0, 0.0)
        elif name == 'psh_nan':
            psh[i] = np.nan
        elif name == 'ps_nan':
            a['PS'][i] = np.nan
        elif name == 't_nan':
            a['T'][3, i] = np.nan
        elif name == 'wind_sign':
            for s in (a, b):
                s['U'][3, i], s['U'][4, i] = 5.0, -5.0
        elif name == 'descending':
            b['PS'][i] = -1000.0
    dtype = np.dtype(dtype)

    def shape(s):
        return dict(PS=s['PS'].reshape(1, 1, n).astype(dtype), **{f: s[f].reshape(1, N, 1, n).astype(dtype) for f in ('T', 'QV', 'U', 'V')})
    plev = PLEV19.copy()
    S = plev.size
    rng = np.random.default_rng(3)
    rec = {v: (rng.standard_normal((2, S, 1, n)) * sc).astype(dtype) for v, sc in zip(VARS, (2.0, 5.0, 1.5, 1.5))}
    rec['ps_hist'] = np.stack([psh, psh]).reshape(2, 1, n).astype(np.float64)       # before == after: the value itself at any instant
    times = np.array(['1995-07-16T12:00:00', '1995-08-16T12:00:00'], dtype='datetime64[s]')
    return dict(ak=ak, bk=bk, plev=plev, a=shape(a), b=shape(b), deltas=rec, times=times, names=names, n_edge=ne,
                target=np.datetime64('2006-08-02T12:00:00'))


def min_distance(ps, ak, bk, plev):
    """Smallest relative distance |pa / p - 1| over all full levels, columns and levels, exact hits left out."""
    with np.errstate(all='ignore'):
        pa = O.hybrid_pressure(ak, bk, _f64(ps))[1]
        r = np.abs(pa[:, :, None] / _f64(plev)[None, None, :, None, None] - 1.0)
    r = r[np.isfinite(r) & (r != 0.0)]
    return r.min() if r.size else np.inf


def conditions():
    """What the cases exist for, asserted on the CPU.  Returns the figures."""
    import points_file_cases
    assert np.array_equal(PLEV5, points_file_cases.PLEV5)
    out = {}
    # caps on NaNs of the statement: a kernel cannot pass by returning NaN.  With these few model levels 100000 Pa lies below
    # the lowest full level in every column: that level is all NaN, every other one has at least 30 % valid columns
    for (grid, nlev, p5), cap in ((((7, 9), 12, True), 0.30), (((10, 10), 20, False), 0.15), (((6, 11), 21, False), 0.15)):
        c = case(grid, nlev, plev5=p5)
        a, b = fields(c['era']), fields(c['b'])
        x = state_on_plev(*a, c['era']['ak'], c['era']['bk'], c['plev'])
        times = {v: c['delta_times'] for v in VARS + ('ps_hist',)}
        change = state_change(a, b, c['era']['ak'], c['era']['bk'], c['plev'])
        err = state_error(a, b, c['era']['ak'], c['era']['bk'], c['plev'], c['deltas'], times, c['target_dt'])
        for name, f in (('state', x), ('change', change), ('error', err)):
            share = np.isnan(f).mean()
            out[(grid, nlev, name)] = share
            assert share <= cap, (grid, nlev, name, share)
            valid = (~np.isnan(f)).mean(axis=(0, 1, 3, 4))
            assert np.all(valid[np.asarray(c['plev']) != np.max(c['plev'])] >= 0.30), (grid, nlev, name, valid)
        assert np.isfinite(x).any() and np.nanmax(np.abs(change)) > 0.0
    # no pa within 1e-9 of a level, except the exact hits
    for ncol in GRIDS:
        for nlev in NLEVS:
            for dtype in ('float64', 'float32'):
                c = case(ncol, nlev, dtype)
                for st in (c['era'], c['b']):
                    d = min_distance(st['PS'], c['era']['ak'], c['era']['bk'], PLEV19)
                    assert d >= MIN_DISTANCE, (ncol, nlev, dtype, d)
        db = case(ncol, 12)['b']['PS'] - case(ncol, 12)['era']['PS']
        assert db.min() >= 50.0 and db.max() <= 300.0
    for hybrid_top in (False, True):
        for n in (None, 66, 96):
            e = edge_case(n, hybrid_top=hybrid_top)
            for st in (e['a'], e['b']):
                assert min_distance(st['PS'], e['ak'], e['bk'], e['plev']) >= MIN_DISTANCE
            assert e['names'][-1] == EDGE_NAMES[-1] and len(e['names']) == (n or len(EDGE_NAMES))
    e = edge_case()
    akm, bkm = O.full_level_coeffs(e['ak'], e['bk'])
    assert akm[2] == 10000.0 and bkm[2] == 0.0 and akm[0] == 1000.0 and bkm[0] == 0.0          # exact pure-pressure full levels
    col = {n: i for i, n in enumerate(e['names'])}
    pa_a = O.hybrid_pressure(e['ak'], e['bk'], e['a']['PS'])[1][0, :, 0]
    pa_b = O.hybrid_pressure(e['ak'], e['bk'], e['b']['PS'])[1][0, :, 0]
    assert pa_a[-1, col['low_in_a']] < 85000.0 < pa_b[-1, col['low_in_a']]
    assert pa_b[-1, col['descending']] < pa_b[0, col['descending']]
    t = edge_case(hybrid_top=True)
    pt_a = O.hybrid_pressure(t['ak'], t['bk'], t['a']['PS'])[1][0, :, 0]
    pt_b = O.hybrid_pressure(t['ak'], t['bk'], t['b']['PS'])[1][0, :, 0]
    assert pt_a[0, col['low_in_a']] < 500.0 < pt_b[0, col['low_in_a']]                         # above the top in state b alone
    return out
