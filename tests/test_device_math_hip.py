"""GPU tests of the device math functions of pgw4era5_amd/csrc/pgw_device.h against exact references (mpmath, 240 bits) and
exact restatements, on the arguments of tests/device_math_cases.py: the three logarithms (pgw_log / pgw_log_f3,
pgw_log_tab, pgw_log_dd), pgw_exp / pgw_exp_finite, and the float64 e_sat fast path with the humidity wrappers built on
it.  tests/test_device_math_host.py holds the CPU side (the table, the restatement against the exact logarithm, the
checker)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import device_math_cases as M                                                         # noqa: E402

pytestmark = pytest.mark.gpu

POPULATIONS = ['structured', 'under_binade', 'near_one', 'limits', 'pressures', 'magnitudes', 'near_one_random']
LOG_ENTRIES = ['pgw_test_log', 'pgw_test_log_table', 'pgw_test_log_f3', 'pgw_test_log_dd']
FLOWS = ['common', 'reference']
_device_results = {}


def _run(entry, x):
    """out[i] = f(x[i]) through a diagnostic entry with the signature of pgw_test_log."""
    from pgw4era5_amd.device import default_context
    ctx = default_context()
    d_in = ctx.to_device(np.ascontiguousarray(x, dtype=np.float64))
    d_out = ctx.empty(x.shape, np.float64)
    ctx._check(getattr(ctx.lib, entry)(ctx.handle, x.size, d_in.ptr, d_out.ptr))
    out = d_out.numpy()
    d_in.free()
    d_out.free()
    return out


def _log(entry, name):
    """One launch per (entry, population), shared by the tests below; read-only."""
    if (entry, name) not in _device_results:
        out = _run(entry, M.log_populations()[name])
        out.setflags(write=False)
        _device_results[entry, name] = out
    return _device_results[entry, name]


def _normal(x):
    with np.errstate(invalid='ignore'):
        return (x >= M.MIN_NORMAL) & (x <= M.MAX_DOUBLE)


def _report(what, name, err, x):
    worst = int(np.nanargmax(err))
    print('%s on %s: %d arguments, max %.4f ulp at %r' % (what, name, err.size, err[worst], x[worst]))
    return err[worst], x[worst]


# ------------------------------------------------------------------ logarithms
@pytest.mark.parametrize('name', POPULATIONS)
def test_log_tab_is_its_restatement_bit_for_bit(name):
    """pgw_log_tab equals its exact restatement (device_math_cases.log_tab_restated: the operations of pgw_device.h with one
    rounding per fma, the table parsed from pgw_log_table.h) in every bit wherever the restatement is defined; elsewhere
    (not a positive normal double, or k = 0 in intervals 79 / 80) it is pgw_log's bits, as the code says.  With
    test_device_math_host.py this bounds the device function's true error by the restatement's: 1.489 ulp measured."""
    got = _log('pgw_test_log_table', name)
    val, ok, _ = M.log_tab_reference(name)
    bad = ok & ~M.same_bits(got, val)
    assert not bad.any(), (bad.sum(), M.log_populations()[name][bad][:5], got[bad][:5], val[bad][:5])
    other = ~ok & ~M.same_bits(got, _log('pgw_test_log', name))
    assert not other.any(), (other.sum(), M.log_populations()[name][other][:5])


@pytest.mark.parametrize('name', POPULATIONS)
def test_log_true_error_is_at_most_one_ulp(name):
    """pgw_log against the exact logarithm on positive normal arguments: <= 1.0 ulp, fdlibm's documented bound (a CPU port
    with 1 / d in place of v_rcp_f64 and its Newton steps measured 0.758).  Measured on the MI355X: 0.7582 ('structured',
    'under_binade'), 0.530 on the pressures; not the correctly rounded double for 1.1 % of the pressures, 2.9 % of
    'structured', 10.5 % of 'under_binade', 0.04 % of 'magnitudes'."""
    x = M.log_populations()[name]
    ok = _normal(x) & (x != 1.0)                                   # ln 1 = 0 has no ulp: the value itself is asserted
    err = np.abs(M.log_reference(name).ulp_error(_log('pgw_test_log', name)))[ok]
    worst, at = _report('pgw_log', name, err, x[ok])
    print('pgw_log on %s: not correctly rounded %.3f %%' % (name, 100 * (_log('pgw_test_log', name)[ok] != M.log_reference(name).rd[ok]).mean()))
    assert not np.isnan(err).any() and worst <= 1.0, (worst, at)
    assert (_log('pgw_test_log', name)[x == 1.0] == 0.0).all()


@pytest.mark.parametrize('name', POPULATIONS)
def test_log_f3_is_log_bit_for_bit(name):
    """pgw_log_f3 (three-address FMA Horner steps) gives pgw_log's bits, non-normal arguments included."""
    bad = ~M.same_bits(_log('pgw_test_log_f3', name), _log('pgw_test_log', name))
    assert not bad.any(), (bad.sum(), M.log_populations()[name][bad][:5])


@pytest.mark.parametrize('name', POPULATIONS)
def test_log_dd_true_error_and_share_correctly_rounded(name):
    """pgw_log_dd against the exact logarithm on positive normal arguments: <= 0.55 ulp (0.5 from the final rounding, the
    fdlibm polynomial's documented 2^-58.45 ~ 0.02 ulp, double-double slop).  On the pressures (uniform 1e-4 .. 1.1e5 Pa)
    at most 1 result in 10^3 is not the correctly rounded double (pgw_device.h states ~3 in 10^4 for this population).
    The other populations only print their share; nothing is asserted of it.  Measured on the MI355X: maximum 0.5127 ulp
    ('structured'; a CPU port with 1 / d for v_rcp_f64 gave 0.515); not correctly rounded 0.0225 % of 'pressures', 0.085 %
    of 'structured', 0.150 % of 'under_binade', 0.005 % of 'magnitudes', none of 'near_one', 'limits', 'near_one_random'."""
    x = M.log_populations()[name]
    ok = _normal(x) & (x != 1.0)
    ref, got = M.log_reference(name), _log('pgw_test_log_dd', name)
    err = np.abs(ref.ulp_error(got))[ok]
    worst, at = _report('pgw_log_dd', name, err, x[ok])
    share = (got[ok] != ref.rd[ok]).mean()
    print('pgw_log_dd on %s: not correctly rounded %.4f %%' % (name, 100 * share))
    assert worst <= 0.55, (worst, at)
    assert (got[x == 1.0] == 0.0).all()
    if name == 'pressures':
        assert share <= 1e-3, share


@pytest.mark.parametrize('entry', LOG_ENTRIES)
def test_logs_on_arguments_outside_the_positive_normal_range(entry):
    """All four logarithms: 0 and -0 -> -inf, negative -> NaN, inf -> inf, NaN -> NaN, denormals within 1 ulp of the exact
    value (the device library's log, which every fast path hands them to)."""
    x = M.log_populations()['limits']
    got, ref = _log(entry, 'limits'), M.log_reference('limits')
    assert (got[x == 0.0] == -np.inf).all() and (x == 0.0).sum() == 2
    assert np.isnan(got[x < 0]).all() and (x < 0).sum() == 2
    assert (got[x == np.inf] == np.inf).all() and np.isnan(got[np.isnan(x)]).all()
    den = (x > 0) & (x < M.MIN_NORMAL)
    assert den.sum() == 3
    err = np.abs(ref.ulp_error(got))[den]
    print(entry, 'denormals', x[den], err)
    assert err.max() <= 1.0, (err, x[den])


# ------------------------------------------------------------------ exponentials
def _exp():
    """pgw_exp over exp_arguments(), one launch shared by the two tests below."""
    if 'pgw_test_exp' not in _device_results:
        from pgw4era5_amd.device import default_context
        ctx = default_context()
        x = M.exp_arguments()
        dx = ctx.to_device(np.ascontiguousarray(x))
        out, lib = ctx.empty(x.shape, np.float64), ctx.empty(x.shape, np.float64)
        ctx._check(ctx.lib.pgw_test_exp(ctx.handle, x.size, dx.ptr, out.ptr, lib.ptr))
        got = out.numpy()
        got.setflags(write=False)
        _device_results['pgw_test_exp'] = got
        for d in (dx, out, lib):
            d.free()
    return _device_results['pgw_test_exp']


def test_exp_true_error_is_at_most_one_ulp():
    """pgw_exp against the exact exponential wherever that is a normal double: <= 1.0 ulp, the device library's documented
    accuracy for exp (whose bits pgw_exp has: test_hip_parity.py::test_device_exp_is_library_exp).  Overflow gives inf,
    underflow below the denormals 0, NaN stays NaN.  Arguments: a3 (T - T0) / (T - a4) of every edge temperature in both
    phases, the specials of that test, 50 000 seeded in (-760, 720)."""
    x, ref, got = M.exp_arguments(), M.exp_reference(), _exp()
    ok = ref.normal()
    err = np.abs(ref.ulp_error(got))[ok]
    worst, at = _report('pgw_exp', 'exp_arguments', err, x[ok])
    assert ok.sum() > 60000 and worst <= 1.0, (worst, at)
    assert (got[ref.rd == np.inf] == np.inf).all() and (got[x < -760] == 0.0).all()
    assert np.isnan(got[np.isnan(x)]).all() and np.isnan(x).sum() >= 3


@pytest.mark.parametrize('group', M.EXP_GROUPS)
def test_exp_finite_is_exp_for_every_finite_argument(group):
    """pgw_exp_finite (no range selects; the exponential of the float64 e_sat fast path) gives pgw_exp's bits for every
    finite argument - those that overflow and underflow included - and for NaN; NaN at +-inf.
    'esat_arguments' reaches |x| = 5.6e19 (the neighbours of the zero divisors T = 32.19 and T = -0.7): beyond |x| ~ 2^50
    n = rint(x log2 e) is off by many units and x - n ln2 is no reduced remainder, which is what the guard on r in
    pgw_exp_impl is for - without it the sign of the saturated result is arbitrary there."""
    sl = M.exp_group(group)
    x, want = M.exp_arguments()[sl], _exp()[sl]
    got = _run('pgw_test_exp_finite', x)
    fin = ~np.isinf(x)
    bad = fin & ~M.same_bits(got, want)
    print('pgw_exp_finite on %s: %d of %d finite arguments differ from pgw_exp' % (group, bad.sum(), fin.sum()))
    for j in np.flatnonzero(bad)[:12]:
        print('   ', repr(x[j]), repr(got[j]), repr(want[j]))
    assert not bad.any(), (bad.sum(), x[bad][:5], got[bad][:5], want[bad][:5])
    assert np.isnan(got[np.isinf(x)]).all() and np.isnan(got[np.isnan(x)]).all()
    if group == 'specials':
        assert np.isinf(x).sum() == 2 and (x[fin] > 1024).any() and (x[fin] < -1075).any()    # beyond both range selects


def test_exp_reduced_is_exp_on_its_range():
    """pgw_exp_reduced (neither selects nor guard; what esat_mixed and the Magnus kernel of step_01 call) gives pgw_exp's
    bits on its stated range |x| <= 1000 - every argument of the three groups in it, overflow above 709.78 and underflow
    below -745.13 included - and NaN for NaN."""
    x, want = M.exp_arguments(), _exp()
    with np.errstate(invalid='ignore'):
        sel = (np.abs(x) <= 1000.0) | np.isnan(x)
    got = _run('pgw_test_exp_reduced', x[sel])
    bad = ~M.same_bits(got, want[sel])
    assert not bad.any(), (bad.sum(), x[sel][bad][:5], got[bad][:5], want[sel][bad][:5])
    assert sel.sum() > 60000 and (want[sel] == np.inf).any() and (want[sel] == 0).any() and np.isnan(got[np.isnan(x[sel])]).all()


# ------------------------------------------------------------------ float64 e_sat and the humidity wrappers
# the three forms of the function-level API: float64 operands in both dtype flows, float32 storage in the default flow
FORMS = [('common', np.float64), ('reference', np.float64), ('common', np.float32)]


@pytest.fixture(params=FORMS, ids=lambda f: '%s-%s' % (f[0], np.dtype(f[1]).name))
def form(request, monkeypatch):
    from pgw4era5_amd import settings
    monkeypatch.setattr(settings, 'function_dtype_flow', request.param[0])
    return request.param


def _esat(ta):
    """(ew, ei, es) of the function-level API."""
    from pgw4era5_amd import functions as F
    pa = np.full_like(ta, 101325.0)
    return (F.saturation_vapor_pressure_water_or_ice(pa, ta, True), F.saturation_vapor_pressure_water_or_ice(pa, ta, False),
            F.saturation_vapor_pressure_water_and_ice(pa, ta))


def _narrow(v, dtype):
    with np.errstate(over='ignore'):
        return v.astype(dtype)


def _esat_literal(ta, ew, ei):
    """alpha e_w + (1 - alpha) e_i of reference functions.py:91-105 in numpy, on the device's own e_w and e_i."""
    alpha = M.alpha_literal(ta)
    with np.errstate(all='ignore'):
        return alpha * ew + (1 - alpha) * ei


def test_esat_fast_path_is_the_literal_expression(form):
    """saturation_vapor_pressure_water_and_ice in float64 (esat_mixed: one phase, div_ns, pgw_exp_reduced; esat_special for
    the mixed range, T <= 40 K and NaN) is alpha e_w + (1 - alpha) e_i as the reference writes it, bit for bit (NaN where
    that is NaN), with alpha formed in numpy as functions.py:91-105 forms it and e_w, e_i from
    saturation_vapor_pressure_water_or_ice (IEEE division, pgw_exp).  Every limit with four neighbours on each side -
    273.16, 250.16, 40.0, the two zero divisors 32.19 and -0.7, 0 - the special values up to 1e300, +-inf, NaN, and
    three sweeps.  (For finite T between 7.96e306 and 1.03e307 the literal expression is NaN and the fast path finite:
    known, not in the list.)  With float32 storage the temperatures are the list rounded to float32, and all three results
    are np.float32 of the float64 values on the widened temperatures: one rounding, bit for bit."""
    flow, dtype = form
    ta = M.temperatures(dtype).astype(np.float64)                  # the temperatures the kernel computes on
    assert (np.abs(ta[np.isfinite(ta)]) <= 1e300).all()
    ew, ei, es = _esat(ta)
    assert es.dtype == np.float64
    want = _esat_literal(ta, ew, ei)
    bad = ~M.same_bits(es, want)
    assert not bad.any(), (bad.sum(), ta[bad][:8], es[bad][:8], want[bad][:8])
    # the list reaches every branch: both one-phase ranges, the mixed range, the cold literal path with its NaN and inf
    assert (ta >= M.T0).sum() > 100 and ((ta <= M.TI) & (ta > 40)).sum() > 100 and ((ta < M.T0) & (ta > M.TI)).sum() > 100
    cold = ta <= 40.0
    assert np.isnan(want[cold]).any() and np.isinf(want[cold]).any() and (want[cold] == 0).any() and (want[cold] > 0).any()
    if dtype == np.float32:
        for got, wide in zip(_esat(M.temperatures(np.float32)), (ew, ei, want)):
            assert got.dtype == np.float32
            bad = ~M.same_bits(got, _narrow(wide, np.float32))
            assert not bad.any(), (bad.sum(), ta[bad][:8])


@pytest.mark.parametrize('flow', FLOWS)
@pytest.mark.parametrize('water', [True, False], ids=['water', 'ice'])
def test_esat_phases_against_the_exact_exponential(flow, water, monkeypatch):
    """e_w and e_i in float64 against 611.21 exp(a3 (T - T0) / (T - a4)) with the argument formed in numpy float64 and the
    exponential and the product exact: <= 2 ulp (1 from pgw_exp, 0.5 from the product's rounding, 0.5 from rounding the
    reference) wherever exp(..) is a normal double - the range for which pgw_exp's 1 ulp holds.  For arguments between
    -714.8 and -708.4 (T near 38 K over water, 8 K over ice) e_sat is still a normal double while exp(..) is a denormal
    one with fewer bits; there pgw_exp's ulp is the denormal spacing 2^-1074, which 611.21 magnifies: bound
    611.21 * 2^-1074 + 1 ulp of the result.  Measured: e_w 0.98 ulp, e_i 1.33 ulp at T = 153.07 K on the first range;
    7.47 ulp (of a bound of 20) at T = 37.98 K over water on the second."""
    from pgw4era5_amd import settings
    monkeypatch.setattr(settings, 'function_dtype_flow', flow)
    ta = M.temperatures()
    dev = _esat(ta)[0 if water else 1]
    ref = M.esat_reference(water)
    exp_normal = M.esat_exp_is_normal(water)
    ok = ref.normal() & exp_normal
    err = np.abs(ref.ulp_error(dev))
    worst, at = _report('e_w' if water else 'e_i', flow, err[ok], ta[ok])
    assert ok.sum() > 9000 and worst <= 2.0, (worst, at)
    low = ref.normal() & ~exp_normal
    if low.any():
        bound = 611.21 * 2.0 ** -1074 / np.spacing(ref.rd[low]) + 1.0
        print('denormal exp: T', ta[low], 'ulp', err[low], 'bound', bound)
        assert (err[low] <= bound).all(), (ta[low], err[low], bound)
    assert low.any() or not water                                  # the cold sweep does reach that range over water


def _check_against_numpy(got, want, domain, elsewhere, what, operands):
    """Bit for bit on `domain`; on `elsewhere` NaN or numpy's value."""
    bad = domain & ~M.same_bits(got, want)
    print('%s: %d of %d elements in the domain, %d differ' % (what, domain.sum(), domain.size, bad.sum()))
    for j in np.flatnonzero(bad)[:12]:
        print('   ', [repr(o[j]) for o in operands], repr(got[j]), repr(want[j]))
    with np.errstate(invalid='ignore'):
        rest = elsewhere & ~domain & ~(np.isnan(got) | (got == want))
    for j in np.flatnonzero(rest)[:12]:
        print('    outside:', [repr(o[j]) for o in operands], repr(got[j]), repr(want[j]))
    assert not bad.any(), (what, bad.sum())
    assert not rest.any(), (what, rest.sum())
    assert domain.sum() > domain.size // 2


def _q_to_rh_numpy(q, pa, es):
    with np.errstate(all='ignore'):
        return (q * pa / (0.622 + 0.378 * q)) / es * 100


def _rh_to_q_numpy(hur, pa, es):
    CON_MW_MD = 0.622
    with np.errstate(all='ignore'):
        vapp = hur / 100 * es                                      # functions.py:123
        return CON_MW_MD * vapp / (pa - (1 - CON_MW_MD) * vapp)    # :66-72


def _wrapper_case(form, fn, literal, first, what):
    """One three-operand wrapper in one form against the numpy float64 expression on the device's own float64 e_sat: bit
    for bit where e_sat is a normal finite double, NaN or numpy's value elsewhere; with float32 storage the operands are
    the float32 roundings, widened for the expression, and the result is np.float32 of its value."""
    flow, dtype = form
    x, pa, ta = M.humidity_operands(first, dtype)
    x64, pa64, ta64 = (v.astype(np.float64) for v in (x, pa, ta))
    es = _esat(ta64)[2]
    got = fn(x, pa, ta)
    assert got.dtype == dtype
    with np.errstate(invalid='ignore'):
        domain = np.isfinite(es) & (np.abs(es) >= M.MIN_NORMAL) & ~(0.622 + 0.378 * x64 == 0)
    elsewhere = (es == 0) | ~np.isfinite(es)                       # a denormal e_sat (T near 7.5 K) is in neither: nothing asserted
    _check_against_numpy(got, _narrow(literal(x64, pa64, es), dtype), domain, elsewhere,
                         '%s (%s, %s)' % (what, flow, np.dtype(dtype).name), (x64, pa64, ta64))


@pytest.mark.parametrize('q', M.HUS_EDGES, ids=[repr(float(v)) for v in M.HUS_EDGES])
def test_specific_to_relative_humidity_is_the_numpy_expression(form, q):
    """specific_to_relative_humidity is (q pa / (0.622 + 0.378 q)) / e_sat * 100 of numpy float64 bit for bit, with the
    device's own e_sat, wherever e_sat is a normal finite double (0.622 + 0.378 q is never zero here).  Where e_sat is 0, inf
    or NaN the result is NaN or numpy's (div_ns alone gives NaN for a zero or infinite divisor where the IEEE division
    gives inf / 0 - its documented behaviour; with v_div_fixup it is numpy's).  Nothing is asserted for a denormal e_sat
    (one temperature of the cold sweep, 7.4998 K): div_ns is not for denormal divisors, the reciprocal overflows.  One case per specific humidity of the edge list, each against
    every pressure of the list at every edge temperature and along the sweeps.
    q = -0.0 gives numpy's -0.0: the two quotients of q -> RH are div_ns followed by v_div_fixup (div_ns_fixup,
    pgw_device.h), which keeps the sign of a zero quotient; div_ns alone turns a -0 numerator into +0."""
    from pgw4era5_amd import functions as F
    _wrapper_case(form, F.specific_to_relative_humidity, _q_to_rh_numpy, q, 'q -> RH, q = %r' % float(q))


@pytest.mark.parametrize('hur', ['edges', 'seeded'])
def test_relative_to_specific_humidity_is_the_numpy_expression(form, hur):
    """relative_to_specific_humidity is vapor_pressure_to_specific_humidity(hur / 100 * e_sat, pa) of numpy float64 bit for
    bit - hur / 100 first, then the product, then the quotient of functions.py:66-72 - on the same domain and with the same
    rule outside it.  'edges': the seven relative humidities of the edge list, which settle the order of the operations.
    'seeded': 509 seeded values in (-50, 200), which hold div_by_100 to the division by 100 on numerators that can show a
    wrong reciprocal (tests/test_device_math_host.py::test_what_the_seeded_hur_can_tell_of_the_reciprocal_of_100: from a
    relative error of 2^-28; the residual step absorbs anything smaller, the last bit of 0.01 included)."""
    from pgw4era5_amd import functions as F
    first = M.HUR_EDGES if hur == 'edges' else M.hur_seeded()
    _wrapper_case(form, F.relative_to_specific_humidity, _rh_to_q_numpy, first, 'RH -> q, %s' % hur)


@pytest.mark.parametrize('mode', ['q_to_rh', 'rh_to_q'])
def test_hybrid_forms_are_the_flat_forms(mode):
    """pgw_specific_to_relative_humidity_hybrid / pgw_relative_to_specific_humidity_hybrid (pa = akm + ps bkm rebuilt in
    registers) on 3 levels of 1 x 8 columns whose T and q / hur rows come from the edge lists (the bottom and top rows
    from the limits of the physical range and the sweeps, the middle row the zero divisors and the special values), one ps
    NaN and one inf: the flat form's bits on pa = akm + ps * bkm built in numpy.  The case can tell a pressure that is
    rounded differently: the flat form on fma(ps, bkm, akm) differs from it in several elements."""
    from pgw4era5_amd import functions as F
    from pgw4era5_amd.device import default_context, dtype_tag
    ctx = default_context()
    ak, bk = np.array([0.0, 4000.0, 6001.0, 0.0]), np.array([0.0, 0.2, 0.9, 1.0])
    akm, bkm = np.array([5000.3, 3000.7, 0.1]), np.array([0.1, 0.55, 0.9975])
    edges, sweeps = M.edge_temperatures()
    n273, n250, n40 = M.neighbours(273.16, 1), M.neighbours(250.16, 1), M.neighbours(40.0, 1)
    ta = np.concatenate([[n273[0], n273[1], n250[1], n250[2], sweeps[0], sweeps[4096], n40[1], n40[2]],
                         [32.19, -0.7, 0.0, -40.0, 1e20, np.inf, np.nan, np.nextafter(32.19, np.inf)],
                         [n273[2], n250[0], sweeps[1], sweeps[4097], sweeps[2], sweeps[4098], sweeps[3], sweeps[4099]]])
    assert np.isin(ta[~np.isnan(ta)], np.concatenate([edges, sweeps])).all() and np.isnan(ta).sum() == 1
    first = M.HUS_EDGES if mode == 'q_to_rh' else M.HUR_EDGES
    x = first[(np.arange(24) + 3) % len(first)]
    ps = np.array([101325.0, 98000.3, np.nan, 1.1e5, np.inf, 55000.7, 1e-4, 101324.9])
    ta, x, ps = ta.reshape(1, 3, 1, 8), x.reshape(1, 3, 1, 8), ps.reshape(1, 1, 8)
    with np.errstate(invalid='ignore'):
        pa = akm[None, :, None, None] + ps[:, None] * bkm[None, :, None, None]
    flat_fn = F.specific_to_relative_humidity if mode == 'q_to_rh' else F.relative_to_specific_humidity
    flat = flat_fn(x, pa, ta)
    ctx.set_levels(ak, bk, akm, bkm)
    dx, dps, dta = ctx.to_device(x), ctx.to_device(ps), ctx.to_device(ta)
    out = ctx.empty(x.shape, np.float64)
    fn = 'pgw_specific_to_relative_humidity_hybrid' if mode == 'q_to_rh' else 'pgw_relative_to_specific_humidity_hybrid'
    ctx._check(getattr(ctx.lib, fn)(ctx.handle, dtype_tag(np.float64), 1, 8, dx.ptr, dps.ptr, dta.ptr, out.ptr))
    got = out.numpy()
    bad = ~M.same_bits(got, flat)
    assert not bad.any(), (bad.sum(), x[bad], pa[bad], ta[bad], got[bad], flat[bad])
    assert np.isfinite(got).sum() >= 8                             # the case is not NaN throughout
    # the power of the case: one rounding instead of two in the pressure is seen
    pa_fma = pa.copy()
    for l in range(3):
        for c in range(8):
            if np.isfinite(ps[0, 0, c]):
                pa_fma[0, l, 0, c] = M.fma(float(ps[0, 0, c]), float(bkm[l]), float(akm[l]))
    seen = (~M.same_bits(flat_fn(x, pa_fma, ta), flat)).sum()
    print('hybrid %s: %d finite results, %d pressures and %d results differ under a fused pressure'
          % (mode, np.isfinite(got).sum(), (pa_fma != pa).sum(), seen))
    assert seen >= 1, seen                                         # measured: 2 (q -> RH) and 4 (RH -> q) of 9 pressures that differ
