"""Edge cases of the step_01 kernels (k_hybrid_to_plev, the error status of both interpolation kernels, k_magnus_rh), shared
by tests/test_step01_edges_host.py (CPU: the stated properties of every case on the oracle alone) and
tests/test_step01_edges_hip.py (GPU).  A plain module: no fixtures, no pytest hooks.

Every builder returns a dict with `ap`, `b` (pressure ascending with the index), `ps` (time, lat, lon), `var` (time, lev, lat,
lon), the target list `targ`, the 4-D pressure field `source_P` = ap + b * ps built in numpy (float64, the construction of
`oracle()` in tests/test_step01_hip.py) and `special`: {flat column index (time, lat, lon order): what sits there}.
`reference(case, targ, mode)` is the oracle on those fields (float64 var: oracle.pgw_oracle, float32 var:
oracle.pgw_oracle_refdtype); `first_error` walks the columns in the reference's order with the oracle's unvectorised loop.
Treat every array as read-only: the results are shared.

Geometry: S <= 12, N <= 16, at most 2 time steps, and 1, 5, 65 (a full wave plus one lane) or 257 (a full block plus one
lane) columns per time step.  `special_positions` puts the special columns where indexing goes wrong: flat column 0 (or 5,
where the smallest reporting column must not be 0), the last lane of a wave, the first lane of the next wave, the first
column of the second time step, the last column (with 257 columns: the single column of the partial last block)."""
import functools
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from oracle import pgw_oracle as O                                                   # noqa: E402
from oracle import pgw_oracle_refdtype as R                                          # noqa: E402

GRIDS = {1: (1, 1), 3: (1, 3), 5: (1, 5), 65: (5, 13), 257: (1, 257)}               # 3: the capacity case only
MODES = ('off', 'linear', 'constant', 'nan')
DTYPES = ('float64', 'float32')
SRC_TEXT = 'Source pressure values must be ascending!'
TARG_TEXT = 'Target pressure values must be ascending!'
OFF_TEXT = 'Extrapolation deactivated but data out of bounds.'
COEFFS = ('usual', 'none_pure', 'all_pure')


# ------------------------------------------------------------------------------------------------ pieces
def coefficients(S, kind='usual'):
    """ap, b, n_pure (pressure ascending with the index, top first).  'usual': b == 0 on the top third; 'none_pure': b[0] > 0;
    'all_pure': every b == 0, the pressure does not depend on ps.  ap + b * ps ascends strictly for 5e4 <= ps <= 1.05e5."""
    k = np.arange(S)
    eta = 0.02 + 0.98 * (k / (S - 1.0))**1.5
    n_pure = max(1, S // 3)
    eta_c = eta[n_pure - 1]
    b = np.where(k < n_pure, 0.0, (np.maximum(eta - eta_c, 0.0) / (1.0 - eta_c))**1.2)
    ap = (eta - b) * 1.0e5
    ap[-1], b[-1] = 0.0, 1.0
    if kind == 'none_pure':
        b[:n_pure] = 1.0e-3 * (k[:n_pure] + 1.0) / n_pure * b[n_pure]
        n_pure = 0
    elif kind == 'all_pure':
        ap, b, n_pure = ap + b * 1.0e5, np.zeros(S), S
    else:
        assert kind == 'usual'
    assert np.all(np.diff(b) >= 0) and int(np.sum(b == 0)) == n_pure and np.all(b[:n_pure] == 0)
    for ps in (5.0e4, 1.05e5):
        assert np.all(np.diff(ap + b * ps) > 0)
    return ap, b, n_pure


def special_positions(ncol, nt, first=0):
    total = ncol * nt
    pos = [first, 63, 64, ncol if nt > 1 else None, total - 1]
    out = []
    for p in pos:
        if p is not None and 0 <= p < total and p not in out:
            out.append(p)
    return out


def field(ap, b, ps, dtype, rng):
    """Temperature-like: a profile plus level noise that scales with the level spacing in ln p (the conditioning argument of
    tests/test_step01_hip.py)."""
    S = len(ap)
    eta = (ap + b * 1.0e5) / 1.0e5
    dln = np.minimum(np.gradient(np.log(ap + b * 1.0e5)), 1.0)
    shape = (ps.shape[0], S) + ps.shape[1:]
    return (200.0 + 90.0 * eta[None, :, None, None] + 2.0 * dln[None, :, None, None] * rng.normal(0, 1.0, shape)).astype(dtype)


def source_pressure(ap, b, ps):
    with np.errstate(invalid='ignore'):
        sp = ap[None, :, None, None] + b[None, :, None, None] * ps[:, None]              # CFday_interp_to_plev.py:91
    assert sp.dtype == np.float64
    return sp


def assemble(ap, b, n_pure, ps, var, targ, special):
    for a in (ap, b, ps, var, targ):
        a.setflags(write=False)
    sp = source_pressure(ap, b, ps)
    sp.setflags(write=False)
    return dict(ap=ap, b=b, n_pure=n_pure, ps=ps, var=var, targ=targ, source_P=sp, special=special)


def healthy_ps(rng, nt, ncol, dtype, lo=5.0e4, hi=1.05e5):
    nlat, nlon = GRIDS[ncol]
    return rng.uniform(lo, hi, (nt, nlat, nlon)).astype(dtype)


def targets(N, lo=1500.0, hi=1.1e5):
    """N ascending pressures from a little above the model top (2000 Pa) to below every surface."""
    return np.geomspace(lo, hi, N)


def target_field(case, targ):
    var = case['var']
    targ = np.asarray(targ, dtype=np.float64)
    return np.ascontiguousarray(np.broadcast_to(targ[None, :, None, None], (var.shape[0], len(targ)) + var.shape[2:]))


def reference(case, targ, mode, fast=True):
    """The oracle on the case's 4-D pressure fields.  fast=False: the unvectorised restatement (float64 oracle only)."""
    var = case['var']
    tp = target_field(case, targ)
    if var.dtype == np.float64 or not fast:
        with np.errstate(invalid='ignore'):
            return O.interp_logp_4d(var, case['source_P'], tp, mode, fast=fast)
    return R.interp_logp_4d(var, case['source_P'], tp, mode)


def first_error(source_P, targ_P, mode, var=None):
    """(text, flat column) of the first column, in the reference's (time, lat, lon) order, at which its serial loop
    (functions.py:493-508: source ends, target ends, then the column's interpolation) raises; None when no column does.
    Which error is raised does not depend on `var`."""
    nt, S, nlat, nlon = source_P.shape
    with np.errstate(invalid='ignore', divide='ignore'):
        lsp, ltp = np.log(source_P), np.log(targ_P)
    if var is None:
        var = np.zeros(source_P.shape)
    tmp = np.zeros((1, targ_P.shape[1], 1, 1))
    flat = 0
    for t in range(nt):
        for j in range(nlat):
            for i in range(nlon):
                cut = (slice(t, t + 1), slice(None), slice(j, j + 1), slice(i, i + 1))
                try:
                    O.interp_1d_for_timelatlon(np.asarray(var[cut], dtype=np.float64), lsp[cut], ltp[cut], tmp, 1, 1, 1, mode)
                except ValueError as e:
                    return str(e), flat
                flat += 1
    return None


def inside_every(case, targ, skip=()):
    """The targets strictly inside the source range of every column (flat indices in `skip` left out)."""
    sp = case['source_P']
    top, bot = sp[:, 0].reshape(-1), sp[:, -1].reshape(-1)
    keep = np.ones(top.shape, dtype=bool)
    keep[list(skip)] = False
    return targ[(targ > top[keep].max()) & (targ < bot[keep].min())]


def restarts(targ):
    """How often the kernels' scan restarts on this list: a target that is not >= its predecessor, where the predecessor of
    the first target is -inf and a NaN target counts as +inf for its successor."""
    with np.errstate(invalid='ignore', divide='ignore'):
        lx = np.log(np.asarray(targ, dtype=np.float64))
    n, prev = 0, -np.inf
    for x in lx:
        if not x >= prev:
            n += 1
        prev = x if x == x else np.inf
    return n


# ------------------------------------------------------------------------------------------------ a. ps
PS_VALUES = (np.nan, np.inf, -np.inf, -3.0e4)


@functools.lru_cache(maxsize=None)
def ps_case(coeff, dtype, ncol=65, first=0):
    """NaN, +inf, -inf and -3e4 Pa in `ps` of the special columns (cycling in that order), healthy columns around them."""
    nt = 2 if ncol == 65 else 1
    S, N = 10, 12
    rng = np.random.default_rng(100 + ncol + first)
    ap, b, n_pure = coefficients(S, coeff)
    ps = healthy_ps(rng, nt, ncol, dtype)
    special = {}
    for n, p in enumerate(special_positions(ncol, nt, first)):
        ps.flat[p] = PS_VALUES[n % 4]
        special[p] = PS_VALUES[n % 4]
    return assemble(ap, b, n_pure, ps, field(ap, b, ps, dtype, rng), targets(N), special)


# ------------------------------------------------------------------------------------------------ b. var
FILL = 1.0e20


@functools.lru_cache(maxsize=None)
def var_case(dtype, ncol=65):
    """NaN at the top level, at the bottom level and at an interior level of different columns, 1e20 at one level of
    another.  special: {flat column: (level, value)}."""
    nt = 2 if ncol == 65 else 1
    S, N = 11, 16
    rng = np.random.default_rng(200 + ncol)
    ap, b, n_pure = coefficients(S)
    ps = healthy_ps(rng, nt, ncol, dtype)
    var = field(ap, b, ps, dtype, rng)
    nlat, nlon = GRIDS[ncol]
    v = var.reshape(nt, S, nlat * nlon)
    what = [(0, np.nan), (S - 1, np.nan), (S // 2, np.nan), (3, FILL), (S // 2 + 1, np.nan)]
    special = {}
    for n, p in enumerate(special_positions(ncol, nt)):
        lev, val = what[n % len(what)]
        v[p // ncol, lev, p % ncol] = val
        special[p] = (lev, val)
    return assemble(ap, b, n_pure, ps, var, targets(N), special)


# ------------------------------------------------------------------------------------------------ c. source order
@functools.lru_cache(maxsize=None)
def equal_levels_case(dtype):
    """Two adjacent pure-pressure levels (1 and 2) of one pressure.  targ holds that pressure (`hit`: its index), a target
    between the pair and the next level (`between`) and targets inside every column."""
    nt, ncol, S = 2, 65, 12
    rng = np.random.default_rng(300)
    ap, b, n_pure = coefficients(S)
    assert n_pure >= 4
    ap[2] = ap[1]
    ps = healthy_ps(rng, nt, ncol, dtype)
    var = field(ap, b, ps, dtype, rng)
    assert np.all(var[:, 1] != var[:, 2])
    between = 0.5 * (ap[2] + ap[3])
    case = assemble(ap, b, n_pure, ps, var, np.zeros(0), {})
    targ =np.sort(np.concatenate([[0.5 * (ap[0] + ap[1]), ap[1], between], inside_every(case, targets(9))]))
    targ.setflags(write=False)
    case.update(targ=targ, hit=int(np.nonzero(targ == ap[1])[0][0]), between=int(np.nonzero(targ == between)[0][0]))
    return case


# ap, b whose levels 4 and 5 cross for ps < 87500 Pa while the ends ascend for every ps >= 5e4
CROSS_AP = np.array([2000.0, 6000.0, 12000.0, 15000.0, 30000.0, 2000.0, 3000.0, 0.0])
CROSS_B = np.array([0.0, 0.0, 0.0, 0.1, 0.3, 0.62, 0.9, 1.0])


@functools.lru_cache(maxsize=None)
def crossing_case(dtype):
    """Even flat columns: ps in [5e4, 5.3e4], levels 4 and 5 out of order; odd ones: ps in [9.5e4, 1.05e5], ascending."""
    nt, ncol = 2, 65
    rng = np.random.default_rng(310)
    ap, b = CROSS_AP.copy(), CROSS_B.copy()
    nlat, nlon = GRIDS[ncol]
    low = rng.uniform(5.0e4, 5.3e4, nt * ncol)
    high = rng.uniform(9.5e4, 1.05e5, nt * ncol)
    ps = np.where(np.arange(nt * ncol) % 2 == 0, low, high).reshape(nt, nlat, nlon).astype(dtype)
    var = field(ap, b, ps, dtype, rng)
    # 36000 and 40000 Pa lie between the crossed levels of every low column: the first match is level 4, not 6
    targ = np.array([1500.0, 4000.0, 9000.0, 18000.0, 30000.0, 36000.0, 40000.0, 47000.0, 49500.0, 62000.0, 90000.0, 1.1e5])
    return assemble(ap, b, 3, ps, var, targ, {p: 'low' for p in range(0, nt * ncol, 2)})


@functools.lru_cache(maxsize=None)
def zero_ps_case(dtype, column=64):
    """ps == 0 in one column: its last level (ap = 0, b = 1) has pressure 0, ln 0 = -inf lies below the first level."""
    nt, ncol, S, N = 2, 65, 10, 12
    rng = np.random.default_rng(320)
    ap, b, n_pure = coefficients(S)
    ps = healthy_ps(rng, nt, ncol, dtype)
    ps.flat[column] = 0.0
    return assemble(ap, b, n_pure, ps, field(ap, b, ps, dtype, rng), targets(N), {column: 0.0})


# ------------------------------------------------------------------------------------------------ d. target lists
NAN = np.nan
LISTS = {
    'duplicates': [3000.0, 50000.0, 50000.0, 20000.0, 20000.0, 90000.0, 90000.0],
    'descends_inside': [3000.0, 60000.0, 90000.0, 10000.0, 30000.0, 70000.0, 95000.0],
    'nan_middle': [3000.0, 40000.0, 85000.0, NAN, 10000.0, 80000.0],
    'nan_first': [NAN, 10000.0, 30000.0, 80000.0],
    'nan_last': [5000.0, 30000.0, 80000.0, NAN],
    'one_nan': [NAN],
}
SORTED_DUPLICATES = [3000.0, 20000.0, 20000.0, 50000.0, 50000.0, 50000.0, 90000.0]   # takes no restart: >= holds
DESCENDING_ENDS = [50000.0, 30000.0, 60000.0, 20000.0]                               # last < first


@functools.lru_cache(maxsize=None)
def list_case(dtype, ncol=65):
    """A healthy case for the target lists above (case['targ'] is a plain sorted list)."""
    nt = 2 if ncol == 65 else 1
    S = 10
    rng = np.random.default_rng(400 + ncol)
    ap, b, n_pure = coefficients(S)
    ps = healthy_ps(rng, nt, ncol, dtype)
    return assemble(ap, b, n_pure, ps, field(ap, b, ps, dtype, rng), targets(12), {})


# ------------------------------------------------------------------------------------------------ e. capacity
@functools.lru_cache(maxsize=None)
def capacity_case(dtype):
    """S == 256 with N == 256 on 3 columns: coefficients and field of tests/test_step01_hip.py, targets a little beyond
    both ends."""
    import test_step01_hip as T
    c = T.make_case(256, 19, np.dtype(dtype), seed=21, nt=1, grid=GRIDS[3])
    sp = c['source_P']
    targ = np.geomspace(0.9 * sp[:, 0].min(), 1.05 * sp[:, -1].max(), 256)
    return assemble(c['ap'], c['b'], c['n_pure'], c['ps'], c['var'], targ, {})


# ------------------------------------------------------------------------------------------------ f. error precedence
P_BELOW = 7.0e4          # below the surface of a 5e4 Pa column, inside every other healthy column (ps >= 9e4)
PS_DESC = 1.0e3          # ap[-1] + ps < ap[0] = 2000 Pa: the ends of such a column descend


@functools.lru_cache(maxsize=None)
def precedence_case(which, dtype):
    """Cases A, B, C and E of an 'off' call.  -> case with `targ`, `expect` = (text, flat column) as the reference's column
    order gives it.  Healthy columns: ps in [9e4, 1.05e5]; `targ`: pressures inside all of them plus P_BELOW (A, B, C), or a
    list with last < first (E)."""
    ncol = 257 if which == 'C' else 65
    S = 10
    rng = np.random.default_rng(500 + ord(which))
    ap, b, n_pure = coefficients(S)
    ps = healthy_ps(rng, 1, ncol, dtype, lo=9.0e4)
    assert PS_DESC < ap[0]
    if which == 'A':
        special = {0: 5.0e4, 5: PS_DESC}
    elif which == 'B':
        special = {0: PS_DESC, 5: 5.0e4}
    elif which == 'C':
        special = {0: 5.0e4, 256: PS_DESC}
    else:
        assert which == 'E'
        special = {0: PS_DESC}
    for p, v in special.items():
        ps.flat[p] = v
    case = assemble(ap, b, n_pure, ps, field(ap, b, ps, dtype, rng), targets(12), special)
    if which == 'E':
        targ = np.array(DESCENDING_ENDS)
    else:
        targ = np.sort(np.concatenate([inside_every(case, np.geomspace(2500.0, 8.9e4, 9), skip=special), [P_BELOW]]))
    targ.setflags(write=False)
    case['targ'] = targ
    case['expect'] = {'A': (OFF_TEXT, 0), 'B': (SRC_TEXT, 0), 'C': (OFF_TEXT, 0), 'E': (SRC_TEXT, 0)}[which]
    return case


@functools.lru_cache(maxsize=None)
def precedence_case_d(both_in_one, dtype):
    """Case D, for interp_logp_4d with a per-column target field.  -> (case, targ_P, expect).
    both_in_one False: column 2's targets have last < first, column 1 has an out-of-range target.
    both_in_one True: column 1 has a descending source AND descending targets (the source check comes first)."""
    ncol, S = 65, 10
    rng = np.random.default_rng(540 + int(both_in_one))
    ap, b, n_pure = coefficients(S)
    ps = healthy_ps(rng, 1, ncol, dtype, lo=9.0e4)
    if both_in_one:
        ps.flat[1] = PS_DESC
    case = assemble(ap, b, n_pure, ps, field(ap, b, ps, dtype, rng), np.geomspace(2500.0, 8.9e4, 9), {})
    tp = target_field(case, case['targ']).copy()
    t = tp.reshape(1, tp.shape[1], ncol)
    if both_in_one:
        t[0, :, 1] = t[0, ::-1, 1]
        expect = (SRC_TEXT, 1)
    else:
        t[0, :, 2] = t[0, ::-1, 2]
        t[0, -1, 1] = 1.2e5
        expect = (OFF_TEXT, 1)
    tp.setflags(write=False)
    return case, tp, expect


# ------------------------------------------------------------------------------------------------ Magnus
MAGNUS_P = np.array([100000.0, 50000.0, 1000.0])
A_SELECT = {'float32': -87.0, 'float64': -700.0}               # k_magnus_rh selects its exp on a > A_SELECT
A_WINDOW = {'float32': (-87.3, -86.7), 'float64': (-702.0, -698.0)}


def magnus_reference(QV, P, T):
    """Emon_convert_hus_to_hur.py:16-21 in numpy, P (plev,) float64 broadcast over (time, plev, lat, lon)."""
    with np.errstate(all='ignore'):
        return 0.263 * P[None, :, None, None] * QV * (np.exp(17.67 * (T - 273.15) / (T - 29.65)))**(-1)


def magnus_exponent(T):
    with np.errstate(all='ignore'):
        return 17.67 * (T - 273.15) / (T - 29.65)


@functools.lru_cache(maxsize=None)
def magnus_case(dtype):
    """T, QV (1, 3, 2, n) of `dtype`, P = MAGNUS_P.  Along the last axis: the window around the kernel's range select, then
    the named temperatures; row 0 of the lat axis has QV > 0, row 1 has QV == 0 at the named temperatures (inf * 0) and
    missing values in QV at ordinary ones.  -> dict(T, QV, P, want, a, e, names={name: index along the last axis})."""
    dt = np.dtype(dtype)
    lo, hi = A_WINDOW[dtype]
    # T(a) = (17.67 * 273.15 - 29.65 a) / (17.67 - a), rising with a
    t_of = lambda a: (17.67 * 273.15 - 29.65 * a) / (17.67 - a)
    window = np.linspace(t_of(lo) + 1e-4 * (t_of(hi) - t_of(lo)), t_of(hi) - 1e-4 * (t_of(hi) - t_of(lo)), 41)
    named = [('overflow_20K', 20.0), ('overflow_25K', 25.0), ('pole', 29.65), ('underflow_30K', 30.0), ('underflow_40K', 40.0),
             ('plain_200K', 200.0), ('plain_250K', 250.0), ('plain_300K', 300.0), ('nan_T', np.nan), ('fill_T', FILL),
             ('plain_273K', 273.15), ('plain_320K', 320.0)]
    t_row = np.concatenate([window, [v for _, v in named]]).astype(dt)
    names = {k: len(window) + i for i, (k, _) in enumerate(named)}
    n = len(t_row)
    T = np.ascontiguousarray(np.broadcast_to(t_row[None, None, None, :], (1, 3, 2, n))).astype(dt)
    rng = np.random.default_rng(600)
    QV = rng.uniform(1e-6, 2e-2, T.shape).astype(dt)
    for k in ('overflow_20K', 'overflow_25K', 'pole', 'underflow_30K', 'underflow_40K', 'nan_T'):
        QV[:, :, 1, names[k]] = 0.0
    QV[:, :, 1, names['plain_200K']] = np.nan
    QV[:, :, 1, names['plain_250K']] = FILL
    QV[:, :, 1, names['plain_300K']] = 0.0
    a = magnus_exponent(T)
    with np.errstate(all='ignore'):
        e = np.exp(a)
    assert a.dtype == dt and e.dtype == dt
    # subnormal guard: the host libm's exp below the smallest normal number is not the reference to pin
    tiny = np.finfo(dt).tiny
    assert not np.any((e != 0) & (np.abs(e) < tiny)), 'a case whose exp is subnormal in %s' % dtype
    want = magnus_reference(QV, MAGNUS_P, T)
    assert want.dtype == np.float64
    out = dict(T=T, QV=QV, P=MAGNUS_P, want=want, a=a, e=e, names=names, window=slice(0, len(window)))
    for v in (T, QV, want, a, e):
        v.setflags(write=False)
    return out
