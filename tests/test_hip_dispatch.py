"""GPU dispatch matrix of the function-level kernels (the functions.py mirror and the hybrid-level C-ABI entries).

Every column kernel is instantiated per storage dtype and per vector width V (columns per thread, `pick_vec` in
csrc/pgw_capi.hip: float32 V = 4 / 2 / 1, float64 V = 2 / 1, chosen from `ncol % V` - the flat kernels from the element
count - and from the 16-byte alignment of every operand).  The matrix runs each entry over both dtypes, grids whose
column count is 0 / 2 (mod 4) or odd (small ones and ones that span several blocks with a partial last block), one and
three time steps, and a level count with a tail for the U = 4 chunk loop, each in three forms: the default dispatch,
`force_vec1`, and operands that start one element past a 16-byte boundary.  It asserts:
  * against the oracle (fp64 on the float64-cast inputs): `hybrid_pressure` and `time_lerp` are the oracle's bits (the
    library builds with -ffp-contract=off and computes in fp64: float32 storage is the oracle's value rounded once); the
    other entries are within this file's fp64 tolerances, and within one float32 ulp of the rounded oracle in float32;
  * across forms: the same bits, NaN positions included (they differ in addressing, not in arithmetic);
  * across time: every time slab of a three-step call is the one-step call on that slab, bit for bit;
  * error location: p_ref below the surface (integ_geopot) / ps_hist above the delta top (vert_interp_delta) in two
    columns of time step 1 is reported at the smaller flat column in every form, and the context computes the same bits
    afterwards.
Also: `pgw_narrow_f64_f32` (float64 fields narrowed on the way into float32 output files) against numpy's conversion."""
import functools

import numpy as np
import pytest

from oracle import pgw_oracle as O

NLEV = 13                    # nlev % 4 != 0: the U = 4 chunk loop of k_integ_geopot has a tail
NT = 3
SEEDS = (21, 22, 23)         # one synthetic case per time step, same grid and nlev (ak / bk depend on nlev only)
REC = 7                      # delta record of each seed
# ncol = 24, 18, 15 (one block) and 1044, 1050, 1073 (several blocks, partial last block): 0 / 2 (mod 4) and odd
GRIDS = [(4, 6), (3, 6), (3, 5), (36, 29), (35, 30), (37, 29)]
DTYPES = ['float32', 'float64']
FORMS = ['default', 'force_vec1', 'misaligned']
T_BEFORE, T_AFTER, T_NEW = (np.datetime64('2006-07-15T12:00:00'), np.datetime64('2006-08-15T12:00:00'),
                            np.datetime64('2006-08-02T03:00:00'))
P_REF = 30000.0
RT_HUM, RT_GEO, RT_VERT, AT_VERT = 1e-12, 1e-11, 1e-10, 1e-13

F32_IDENTICAL = {}           # entry -> [float32 results equal to the rounded oracle, float32 results]


def pick_vec(dtype, n, aligned=True, force_vec1=False, max_v=4):
    """Python mirror of pick_vec (csrc/pgw_capi.hip)."""
    v = min(2 if np.dtype(dtype) == np.float64 else 4, max_v)
    if force_vec1 or not aligned:
        return 1
    while v > 1 and n % v:
        v >>= 1
    return v


@pytest.fixture(scope='module')
def ctx():
    from pgw4era5_amd.device import default_context
    c = default_context()
    yield c
    if F32_IDENTICAL:
        print('\nfloat32 results bit-identical to the rounded oracle: ' +
              ', '.join('%s %d/%d (%.1f %%)' % (k, a, b, 100.0 * a / b) for k, (a, b) in sorted(F32_IDENTICAL.items())))


@functools.lru_cache(maxsize=None)
def _stack(grid, dtype):
    """NT synthetic cases on one grid stacked along time, in the storage dtype; the pressures the entries take as input
    are the oracle's fp64 values stored in that dtype."""
    from pgw4era5_amd import synthetic
    dt = np.dtype(dtype)
    cs = [synthetic.make_case(nlat=grid[0], nlon=grid[1], nlev=NLEV, seed=s, dtype=dt) for s in SEEDS]
    era = cs[0]['era']
    s = dict(ak=era['ak'], bk=era['bk'], plev=cs[0]['plev'], level1=era['level1'])
    for k in ('PS', 'FIS', 'T', 'QV', 'U', 'V'):
        s[k] = np.ascontiguousarray(np.concatenate([c['era'][k] for c in cs]))
    for k in ('ta', 'tas', 'ps_hist'):
        s[k] = np.ascontiguousarray(np.stack([c['deltas'][k][REC] for c in cs]))
    pa_hl, pa = O.hybrid_pressure(s['ak'], s['bk'], s['PS'].astype(np.float64))
    s['pa_hl'], s['pa'] = pa_hl.astype(dt), pa.astype(dt)
    s['RH'] = O.specific_to_relative_humidity(s['QV'].astype(np.float64), pa, s['T'].astype(np.float64)).astype(dt)
    rng = np.random.default_rng(grid[0] * 100 + grid[1])
    s['pref'] = rng.uniform(2.0e4, 4.5e4, s['PS'].shape).astype(dt)          # per-column p_ref in the storage dtype
    s['pref64'] = rng.uniform(2.0e4, 4.5e4, s['PS'].shape)                   # the fp64 field of pgw_phi_ref_hybrid
    for v in s.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return s


def _f64(x):
    return np.asarray(x, dtype=np.float64)


def _host(x):
    from pgw4era5_amd.device import DeviceArray
    return x.numpy() if isinstance(x, DeviceArray) else np.asarray(x)


def _dev(ctx, x):
    from pgw4era5_amd.device import DeviceArray
    return x if isinstance(x, DeviceArray) else ctx.to_device(np.ascontiguousarray(x))


def _misaligned(ctx, host):
    """A DeviceArray holding `host` that starts one element past the (256-byte aligned) start of a buffer one element
    longer: element-aligned, not 16-byte aligned."""
    from pgw4era5_amd.device import DeviceArray
    host = np.ascontiguousarray(host)
    base = ctx.empty((host.size + 1,), host.dtype)
    d = DeviceArray(ctx, host.shape, host.dtype, ptr=base.ptr + host.dtype.itemsize, owner=base)
    assert d.ptr % 16 != 0 and d.ptr + d.nbytes == base.ptr + base.nbytes
    return d.copy_from(host)


# ------------------------------------------------------------------ the entries
# Each entry: `fields` (the per-time operands, leading axis = time), `call(ctx, ops, nt)` -> tuple of outputs with a leading
# time axis, `oracle(ops)` -> tuple of fp64 values, `check` ('exact' / 'close'), `tol` (fp64 rtol, atol), `flat` (V from the
# element count instead of ncol), `max_v`, `out_f64` (fp64 output whatever the storage dtype).
class Entry:
    def __init__(self, fields, call, oracle, check='close', tol=(RT_HUM, 0.0), flat=False, max_v=4, out_f64=False, vec=True):
        self.fields, self.call, self.oracle, self.check, self.tol = fields, call, oracle, check, tol
        self.flat, self.max_v, self.out_f64, self.vec = flat, max_v, out_f64, vec


def _hybrid_pressure(s):
    from pgw4era5_amd import functions as F
    return Entry(['PS'], lambda ctx, o, nt: F.hybrid_pressure(s['ak'], s['bk'], o['PS']),
                 lambda o: O.hybrid_pressure(s['ak'], s['bk'], _f64(o['PS'])), check='exact')


def _q_to_rh(s):
    from pgw4era5_amd import functions as F
    return Entry(['QV', 'pa', 'T'], lambda ctx, o, nt: (F.specific_to_relative_humidity(o['QV'], o['pa'], o['T']),),
                 lambda o: (O.specific_to_relative_humidity(_f64(o['QV']), _f64(o['pa']), _f64(o['T'])),), flat=True)


def _rh_to_q(s):
    from pgw4era5_amd import functions as F
    return Entry(['RH', 'pa', 'T'], lambda ctx, o, nt: (F.relative_to_specific_humidity(o['RH'], o['pa'], o['T']),),
                 lambda o: (O.relative_to_specific_humidity(_f64(o['RH']), _f64(o['pa']), _f64(o['T'])),), flat=True)


def _humidity_hybrid(s, mode):
    """pgw_{specific_to_relative,relative_to_specific}_humidity_hybrid: pa = akm + ps*bkm rebuilt in registers."""
    from pgw4era5_amd.device import dtype_tag
    x = 'QV' if mode == 'q_to_rh' else 'RH'
    fn = 'pgw_specific_to_relative_humidity_hybrid' if mode == 'q_to_rh' else 'pgw_relative_to_specific_humidity_hybrid'

    def call(ctx, o, nt):
        ctx.set_levels(s['ak'], s['bk'])
        dx, dps, dta = _dev(ctx, o[x]), _dev(ctx, o['PS']), _dev(ctx, o['T'])
        out = ctx.empty(dx.shape, dx.dtype)
        ctx._check(getattr(ctx.lib, fn)(ctx.handle, dtype_tag(dx.dtype), nt, dx.shape[2] * dx.shape[3], dx.ptr, dps.ptr,
                                         dta.ptr, out.ptr))
        return (out.numpy(),)

    def oracle(o):
        _, pa = O.hybrid_pressure(s['ak'], s['bk'], _f64(o['PS']))
        f = O.specific_to_relative_humidity if mode == 'q_to_rh' else O.relative_to_specific_humidity
        return (f(_f64(o[x]), pa, _f64(o['T'])),)
    return Entry([x, 'PS', 'T'], call, oracle)


def _integ_geopot(s, pref, full):
    from pgw4era5_amd import functions as F
    fields = ['pa_hl', 'FIS', 'T', 'QV'] + (['pref'] if pref == 'field' else [])

    def call(ctx, o, nt):
        p = o['pref'] if pref == 'field' else P_REF
        return (F.integ_geopot(o['pa_hl'], o['FIS'], o['T'], o['QV'], s['level1'], p, full_column=full),)

    def oracle(o):
        p = _f64(o['pref']) if pref == 'field' else P_REF
        return (O.integ_geopot(_f64(o['pa_hl']), _f64(o['FIS']), _f64(o['T']), _f64(o['QV']), s['level1'], p),)
    return Entry(fields, call, oracle, tol=(RT_GEO, 0.0))


def _phi_ref_hybrid(s, pref):
    """pgw_phi_ref_hybrid: phi_ref of the ERA state with pa_hl rebuilt in registers; fp64 output, V at most 2."""
    from pgw4era5_amd.device import dtype_tag
    fields = ['T', 'QV', 'PS', 'FIS'] + (['pref64'] if pref == 'field' else [])

    def call(ctx, o, nt):
        ctx.set_levels(s['ak'], s['bk'])
        d = {k: _dev(ctx, o[k]) for k in fields}
        out = ctx.empty(d['PS'].shape, np.float64)
        pf = d['pref64'].ptr if pref == 'field' else None
        ctx._check(ctx.lib.pgw_phi_ref_hybrid(ctx.handle, dtype_tag(d['T'].dtype), nt, d['PS'].shape[1] * d['PS'].shape[2],
                                              d['T'].ptr, d['QV'].ptr, d['PS'].ptr, d['FIS'].ptr, P_REF, pf, out.ptr))
        return (out.numpy(),)

    def oracle(o):
        pa_hl, _ = O.hybrid_pressure(s['ak'], s['bk'], _f64(o['PS']))
        p = _f64(o['pref64']) if pref == 'field' else P_REF
        return (O.integ_geopot(pa_hl, _f64(o['FIS']), _f64(o['T']), _f64(o['QV']), s['level1'], p),)
    return Entry(fields, call, oracle, tol=(RT_GEO, 0.0), max_v=2, out_f64=True)


def _x_lerp():
    ns = 'datetime64[ns]'
    return (float((T_AFTER.astype(ns) - T_BEFORE.astype(ns)).astype(np.int64)),
            float((T_NEW.astype(ns) - T_BEFORE.astype(ns)).astype(np.int64)))


def _time_lerp(s):
    from pgw4era5_amd import functions as F
    x_hi, x_new = _x_lerp()
    return Entry(['T', 'U'], lambda ctx, o, nt: (F.time_lerp(o['T'], o['U'], x_hi, x_new),),
                 lambda o: (O.time_lerp(_f64(o['T']), _f64(o['U']), T_BEFORE, T_AFTER, T_NEW),), check='exact', flat=True)


def _vert_interp_delta(s, sfc):
    from pgw4era5_amd import functions as F
    fields = ['ta', 'pa'] + (['tas', 'ps_hist'] if sfc else [])

    def call(ctx, o, nt):
        return (F.vert_interp_delta(o['ta'], o['pa'], o['tas'] if sfc else None, o['ps_hist'] if sfc else None,
                                    ignore_top_pressure_error=True, plev=s['plev']),)

    def oracle(o):
        return (O.vert_interp_delta(_f64(o['ta']), s['plev'], _f64(o['pa']), _f64(o['tas']) if sfc else None,
                                    _f64(o['ps_hist']) if sfc else None, ignore_top_pressure_error=True),)
    return Entry(fields, call, oracle, tol=(RT_VERT, AT_VERT), vec=False)


ENTRIES = {
    'hybrid_pressure': _hybrid_pressure,
    'specific_to_relative_humidity': _q_to_rh,
    'relative_to_specific_humidity': _rh_to_q,
    'specific_to_relative_humidity_hybrid': lambda s: _humidity_hybrid(s, 'q_to_rh'),
    'relative_to_specific_humidity_hybrid': lambda s: _humidity_hybrid(s, 'rh_to_q'),
    'integ_geopot_scalar_full': lambda s: _integ_geopot(s, 'scalar', True),
    'integ_geopot_scalar_early_exit': lambda s: _integ_geopot(s, 'scalar', False),
    'integ_geopot_field_full': lambda s: _integ_geopot(s, 'field', True),
    'integ_geopot_field_early_exit': lambda s: _integ_geopot(s, 'field', False),
    'phi_ref_hybrid_scalar': lambda s: _phi_ref_hybrid(s, 'scalar'),
    'phi_ref_hybrid_field': lambda s: _phi_ref_hybrid(s, 'field'),
    'time_lerp': _time_lerp,
    'vert_interp_delta_sfc': lambda s: _vert_interp_delta(s, True),
    'vert_interp_delta': lambda s: _vert_interp_delta(s, False),
}


def _vec(e, grid, dtype, nt, form):
    """V of the launch (the pick_vec mirror); 1 for kernels without a vector form."""
    if not e.vec:
        return 1
    ncol = grid[0] * grid[1]
    n = nt * NLEV * ncol if e.flat else ncol
    return pick_vec(dtype, n, aligned=form != 'misaligned', force_vec1=form == 'force_vec1', max_v=e.max_v)


def _run(ctx, e, s, form, t=None):
    """One call of entry `e` in dispatch form `form`, on all NT time steps (t None) or on time slab t alone."""
    ops = {k: (s[k] if t is None else s[k][t:t + 1]) for k in e.fields}
    nt = NT if t is None else 1
    if form == 'misaligned':
        ops = {k: _misaligned(ctx, v) for k, v in ops.items()}
    old = ctx.set_option('force_vec1', 1) if form == 'force_vec1' else None
    try:
        out = e.call(ctx, ops, nt)
    finally:
        if old is not None:
            ctx.set_option('force_vec1', old)
    return tuple(_host(x) for x in out)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype == np.float64 else np.uint32)


def _assert_same_bits(a, b, msg):
    assert a.dtype == b.dtype and a.shape == b.shape, msg
    np.testing.assert_array_equal(_bits(a), _bits(b), err_msg=msg)


def _assert_within_one_ulp(got, want64, msg):
    """float32 `got` is the fp64 oracle rounded once to float32, or one of that value's two float32 neighbours (the ulp
    on each side is the float32 spacing there, which differs at a power of two)."""
    r = want64.astype(np.float32)
    nan = np.isnan(r)
    np.testing.assert_array_equal(np.isnan(got), nan, err_msg=msg + ': NaN positions')
    g, r = got[~nan], r[~nan]
    ok = (g == r) | (g == np.nextafter(r, np.float32(np.inf))) | (g == np.nextafter(r, np.float32(-np.inf)))
    if not ok.all():
        i = np.flatnonzero(~ok)[:5]
        raise AssertionError('%s: %d of %d values more than 1 float32 ulp from the rounded oracle, e.g. got %s want %s (fp64 %s)'
                             % (msg, (~ok).sum(), ok.size, g[i], r[i], want64[~nan][i]))
    return int((g == r).sum()), g.size


def _check_oracle(name, e, dtype, got, want):
    for k, (g, w) in enumerate(zip(got, want)):
        msg = '%s output %d' % (name, k)
        out_dt = np.float64 if e.out_f64 else np.dtype(dtype)
        assert g.dtype == out_dt, (msg, g.dtype)
        w = np.asarray(w, dtype=np.float64)
        assert g.shape == w.shape, (msg, g.shape, w.shape)
        if e.check == 'exact':
            _assert_same_bits(g, w.astype(g.dtype), msg + ': the oracle\'s bits')
        elif g.dtype == np.float32:
            same, total = _assert_within_one_ulp(g, w, msg)
            acc = F32_IDENTICAL.setdefault(name, [0, 0])
            acc[0] += same
            acc[1] += total
        else:
            np.testing.assert_allclose(g, w, rtol=e.tol[0], atol=e.tol[1], equal_nan=True, err_msg=msg)


def test_matrix_reaches_every_vector_width():
    """The matrix below launches every (dtype, V) instance each entry has: float32 V = 4, 2, 1 and float64 V = 2, 1 (V = 2,
    1 for both where the width is capped at 2), both for one and for three time steps."""
    for name, make in ENTRIES.items():
        e = make(dict(ak=None, bk=None, plev=None, level1=None))
        for nt in (1, NT):
            got = {(dt, _vec(e, g, dt, nt, f)) for dt in DTYPES for g in GRIDS for f in FORMS}
            want = {('float32', v) for v in (4, 2, 1) if v <= e.max_v} | {('float64', 2), ('float64', 1)}
            if not e.vec:
                want = {('float32', 1), ('float64', 1)}
            assert got == want, (name, nt, sorted(got))


@pytest.mark.gpu
@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('grid', GRIDS, ids=['%dx%d' % g for g in GRIDS])
@pytest.mark.parametrize('name', list(ENTRIES))
def test_dispatch_matrix(ctx, name, grid, dtype):
    s = _stack(grid, dtype)
    e = ENTRIES[name](s)
    res = {f: _run(ctx, e, s, f) for f in FORMS}
    tag = '%s %s %s' % (name, grid, dtype)
    for f in FORMS[1:]:
        for a, b in zip(res['default'], res[f]):
            _assert_same_bits(b, a, '%s: %s form vs default (V=%d vs %d)' % (tag, f, _vec(e, grid, dtype, NT, f),
                                                                              _vec(e, grid, dtype, NT, 'default')))
    _check_oracle(name, e, dtype, res['default'], e.oracle({k: s[k] for k in e.fields}))
    for t in range(NT):
        one = _run(ctx, e, s, 'default', t)
        for a, b in zip(res['default'], one):
            _assert_same_bits(b, a[t:t + 1], '%s: time slab %d alone vs in the three-step call' % (tag, t))


def _two_columns(ncol):
    """Two columns of one time step: the last one (in the partial last block / last vector group) and lane 1 of a vector
    group in the middle."""
    return ncol - 1, 4 * (ncol // 8) + 1


@pytest.mark.gpu
@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('grid', GRIDS, ids=['%dx%d' % g for g in GRIDS])
@pytest.mark.parametrize('name', ['integ_geopot_field_full', 'integ_geopot_field_early_exit', 'vert_interp_delta_sfc'])
def test_error_column_in_every_form(ctx, name, grid, dtype):
    s = dict(_stack(grid, dtype))
    e = ENTRIES[name](s)
    ncol = grid[0] * grid[1]
    good = _run(ctx, e, s, 'default')
    c1, c2 = _two_columns(ncol)
    if name.startswith('integ_geopot'):
        key, value = 'pref', 2.0e5                   # p_ref below the surface: no half level at or above it
    else:
        key, value = 'ps_hist', 50.0                 # HIST surface pressure above the top delta level
    bad = s[key].copy()
    bad[1].reshape(-1)[[c1, c2]] = value
    s_bad = dict(s, **{key: bad})
    with pytest.raises((ValueError, KeyError)) as want:
        e.oracle({k: s_bad[k] for k in e.fields})
    assert want.type is ValueError
    for f in FORMS:
        with pytest.raises(ValueError) as got:
            _run(ctx, e, s_bad, f)
        assert str(got.value) == str(want.value), (f, str(got.value))
        assert got.value.column == ncol + min(c1, c2), (f, got.value.column)
        after = _run(ctx, e, s, 'default')
        for a, b in zip(good, after):
            _assert_same_bits(b, a, '%s: first valid call after the error (%s form)' % (name, f))


# ------------------------------------------------------------------ pgw_narrow_f64_f32
def _narrow_values(n, seed):
    f32 = np.finfo(np.float32)
    fmax = float(f32.max)
    tie_max = 2.0 ** 128 - 2.0 ** 103                # FLT_MAX + 1/2 ulp: rounds to even, i.e. up to infinity
    tiny = float(f32.tiny)                           # smallest normal 2^-126
    sub = 2.0 ** -149                                # smallest subnormal
    special = [0.0, -0.0, np.inf, -np.inf, np.nan, -np.nan, fmax, -fmax,
               np.nextafter(tie_max, 0.0), tie_max, np.nextafter(tie_max, np.inf), -np.nextafter(tie_max, 0.0), -tie_max,
               1.0e39, -1.0e300, tiny, -tiny, np.nextafter(tiny, 0.0), tiny - sub / 2, tiny * 0.75,
               sub, -sub, sub / 2, np.nextafter(sub / 2, 1.0), np.nextafter(sub / 2, 0.0), 1.5 * sub, 2.5 * sub, sub / 4,
               -3.5 * sub, 1.0e-46, 1.0e-50, -1.0e-300,
               1.0 + 2.0 ** -24, 1.0 + 3 * 2.0 ** -24, -(1.0 + 2.0 ** -24), 1.0 + 2.0 ** -24 + 2.0 ** -52,
               1.0 + 2.0 ** -24 - 2.0 ** -53, 3.0 * 2.0 ** 100 + 2.0 ** 77, 0.1, -1.0 / 3.0, 16777217.0, -16777219.0]
    rng = np.random.default_rng(seed)
    x = rng.choice([-1.0, 1.0], n) * 10.0 ** rng.uniform(-50.0, 45.0, n)
    x[::7] = rng.normal(size=x[::7].shape) * 300.0
    sp = np.asarray(special)
    k = min(n, len(sp))
    x[:k] = sp[:k]
    if n > 2 * len(sp):
        x[-len(sp):] = sp                            # the tail element of the pairwise path is a special value too
    return x


@pytest.mark.gpu
@pytest.mark.parametrize('offset', [0, 8], ids=['aligned', 'offset8'])
@pytest.mark.parametrize('big_endian', [False, True], ids=['le', 'be'])
@pytest.mark.parametrize('n', [1, 2, 3, 1023, 65541])
def test_narrow_f64_f32_matches_numpy(ctx, n, big_endian, offset):
    """float64 -> float32 in the file's byte order: numpy's IEEE round-to-nearest-even conversion, bit for bit - overflow
    to infinity from FLT_MAX + 1/2 ulp on, subnormal results kept (not flushed), ties to even; NaN stays NaN.  offset 8:
    a source that is not 16-byte aligned takes the element-wise path."""
    from pgw4era5_amd.device import DeviceArray
    src = _narrow_values(n, n)
    base = ctx.empty((n + 1,), np.float64)
    d = DeviceArray(ctx, (n,), np.float64, ptr=base.ptr + offset, owner=base).copy_from(src)
    out = ctx.zeros((n,), np.float32)
    ctx._check(ctx.lib.pgw_narrow_f64_f32(ctx.handle, n, d.ptr, out.ptr, 1 if big_endian else 0))
    dt = np.dtype('>f4' if big_endian else '<f4')
    with np.errstate(over='ignore'):
        want = src.astype(dt)
    got = np.frombuffer(out.numpy().tobytes(), dtype=dt)
    nan = np.isnan(src)
    assert np.isnan(got[nan]).all()
    gb = np.frombuffer(got.tobytes(), np.uint8).reshape(n, 4)[~nan]
    wb = np.frombuffer(want.tobytes(), np.uint8).reshape(n, 4)[~nan]
    bad = np.flatnonzero((gb != wb).any(axis=1))
    assert bad.size == 0, 'first mismatches: src %s got %s want %s' % (src[~nan][bad[:5]], got[~nan][bad[:5]], want[~nan][bad[:5]])
