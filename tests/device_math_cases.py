"""Shared by tests/test_device_math_host.py and tests/test_device_math_hip.py (no GPU here): what the device math functions
of pgw4era5_amd/csrc/pgw_device.h are held to.

* exact references: ln and exp of a double from mpmath at 240 bits - the correctly rounded double and what is left of the
  exact value beyond it, so that the error of any candidate comes out in ulps of the correctly rounded result;
* the arguments: populations built from bit patterns (every table interval of pgw_log_tab at its ends, the arguments whose
  logarithm lies just under a binade, the neighbourhood of 1, the limits of the fast paths);
* an exact restatement of pgw_log_tab: the operations of pgw_device.h in their order, every fma one rounding, the table
  parsed from pgw_log_table.h;
* the edge temperatures and operands of the float64 humidity chain.

Every population and every reference is computed once per process (functools.lru_cache) and must not be modified."""
import functools
import os
import re
import struct

import numpy as np
from mpmath import mp, mpf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'pgw4era5_amd', 'csrc')
PREC = 240                                  # bits; the hardest double logarithms need ~120
MIN_NORMAL = 2.2250738585072014e-308
MAX_DOUBLE = 1.7976931348623157e308


# ------------------------------------------------------------------ bit patterns
def bits_of(x):
    return struct.unpack('<Q', struct.pack('<d', x))[0]


def from_bits(b):
    return struct.unpack('<d', struct.pack('<Q', b))[0]


def neighbours(x, n):
    """The n doubles below x, x, and the n doubles above, ascending."""
    x = np.float64(x)
    below, above = [], []
    lo = hi = x
    for _ in range(n):
        lo = np.nextafter(lo, -np.inf)
        hi = np.nextafter(hi, np.inf)
        below.append(lo)
        above.append(hi)
    return np.array(below[::-1] + [x] + above, dtype=np.float64)


def same_bits(a, b):
    """Elementwise: the same bit pattern, or NaN in both (NaN payloads are not compared)."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.dtype == b.dtype and a.shape == b.shape, (a.dtype, b.dtype, a.shape, b.shape)
    u = np.uint64 if a.dtype == np.float64 else np.uint32
    return (a.view(u) == b.view(u)) | (np.isnan(a) & np.isnan(b))


# ------------------------------------------------------------------ exact references
class Exact:
    """Exact values to double-double accuracy: `rd` the correctly rounded doubles, `rest` = exact - rd (itself rounded
    to double: relative 2^-53 of a quantity below half an ulp)."""

    def __init__(self, rd, rest):
        self.rd, self.rest = rd, rest
        self.rd.setflags(write=False)
        self.rest.setflags(write=False)

    def ulp_error(self, cand):
        """Signed error of `cand` in ulps of the correctly rounded double (np.spacing(|rd|)); NaN where rd is not finite
        or zero.  cand - rd is exact for candidates within a factor 2 of rd (Sterbenz)."""
        with np.errstate(all='ignore'):
            ulp = np.spacing(np.abs(self.rd))
            e = ((np.asarray(cand, dtype=np.float64) - self.rd) - self.rest) / ulp
        return np.where(np.isfinite(self.rd) & (self.rd != 0), e, np.nan)

    def normal(self):
        return np.isfinite(self.rd) & (np.abs(self.rd) >= MIN_NORMAL)


def _exact(values, fn):
    rd = np.empty(len(values))
    rest = np.zeros(len(values))
    with mp.workprec(PREC):
        for j, v in enumerate(values):
            y = fn(v)
            if y is None:
                rd[j] = np.nan
                continue
            if isinstance(y, float):
                rd[j] = y
                continue
            r = float(y)                     # mpmath rounds to nearest even
            rd[j] = r
            if np.isfinite(r):
                rest[j] = float(y - mpf(r))
    return Exact(rd, rest)


def _ln(x):
    x = float(x)
    if not x > 0 or x == np.inf:
        return None if (x != x or x < 0) else (-np.inf if x == 0 else np.inf)
    return mp.log(mpf(x))


def _exp(scale):
    def f(x):
        x = float(x)
        if x != x:
            return None
        if x > 720.0:                        # beyond the doubles on either side; mpmath would build huge exponents
            return np.inf
        if x < -760.0:
            return 0.0
        return mpf(scale) * mp.exp(mpf(x))
    return f


def exact_log(x):
    """Exact ln of every double of x (Exact; NaN for negative and NaN, -inf at 0, inf at inf)."""
    return _exact(np.asarray(x, dtype=np.float64), _ln)


def exact_exp(x, scale=1.0):
    """Exact scale * exp(x) for doubles x, `scale` a double taken exactly (Exact; NaN for NaN)."""
    return _exact(np.asarray(x, dtype=np.float64), _exp(float(scale)))


# ------------------------------------------------------------------ the table and the restatement of pgw_log_tab
TAB_OFF_HI = 0x3FE60000                      # high word of 0.6875, the start of interval 0 for k = 0
LN2_HI_TAB, LN2_LO_TAB = float.fromhex('0x1.62e42fefa3800p-1'), float.fromhex('0x1.ef35793c76730p-45')
POLY = [float.fromhex(h) for h in ('0x1.2492492492492p-3', '-0x1.5555555555555p-3', '0x1.999999999999ap-3', '-0x1.0p-2',
                                   '0x1.5555555555555p-2', '-0x1.0p-1')]


@functools.lru_cache(maxsize=None)
def log_table_text():
    """The hexadecimal literals of pgw_log_table.h's body, in order."""
    txt = open(os.path.join(CSRC, 'pgw_log_table.h')).read()
    body = txt[txt.index('#else'):txt.rindex('#endif')]
    return tuple(re.findall(r'-?0x[0-9a-f]\.[0-9a-f]+p[+-]\d+', body))


@functools.lru_cache(maxsize=None)
def log_table():
    """((invc, logc), ...) of pgw_log_table.h."""
    v = [float.fromhex(h) for h in log_table_text()]
    return tuple(zip(v[0::2], v[1::2]))


def interval_hi_word(i, k=0):
    """High word of the first double of table interval i in binade k."""
    return TAB_OFF_HI + (i << 13) + (k << 20)


def interval_ends(i, k=0):
    """First and last double of table interval i in binade k."""
    hw = interval_hi_word(i, k)
    return from_bits(hw << 32), from_bits(((hw + 0x2000) << 32) - 1)


def fma(a, b, c):
    """a * b + c with one rounding, for finite doubles (exact integer arithmetic; python's int / int is correctly
    rounded, which is what float(Fraction(a) * Fraction(b) + Fraction(c)) computes too)."""
    na, da = a.as_integer_ratio()
    nb, db = b.as_integer_ratio()
    nc, dc = c.as_integer_ratio()
    n = na * nb * dc + nc * da * db
    if n == 0:                               # signed zero as IEEE: only (+0) + (-0) and exact cancellation give +0
        return a * b + c
    return n / (da * db * dc)


NOT_RESTATED = None


def log_tab_restated(x):
    """pgw_log_tab(x) operation by operation: (result, w), or (NOT_RESTATED, None) where the device function goes to the
    fdlibm kernel (x not a positive normal finite double, or k == 0 and interval 79 or 80), whose reciprocal instruction
    is not bit-specified."""
    tab = log_table()
    b = bits_of(float(x))
    hi, lo32 = b >> 32, b & 0xFFFFFFFF
    thi = (hi - TAB_OFF_HI) & 0xFFFFFFFF
    i = (thi >> 13) & 127
    k = (thi >> 20) - (0x1000 if thi & 0x80000000 else 0)          # arithmetic shift of the int32
    if not ((hi - 0x00100000) & 0xFFFFFFFF) < 0x7FE00000 or (k == 0 and i in (79, 80)):
        return NOT_RESTATED, None
    z = from_bits((((hi - (thi & 0xFFF00000)) & 0xFFFFFFFF) << 32) | lo32)
    invc, logc = tab[i]
    r = fma(z, invc, -1.0)
    kd = float(k)
    w = fma(kd, LN2_HI_TAB, logc)
    h = w + r
    lo = fma(kd, LN2_LO_TAB, (w - h) + r)
    r2 = r * r
    p = fma(r, POLY[0], POLY[1])
    for c in POLY[2:]:
        p = fma(r, p, c)
    return fma(r2, p, lo) + h, w


# ------------------------------------------------------------------ arguments of the logarithms
LOG_KS = (-1022, -600, -14, -1, 0, 1, 6, 13, 16, 17, 600, 1023)
LOG_LIMITS = np.array([MIN_NORMAL, np.nextafter(MIN_NORMAL, 0.0), MAX_DOUBLE, 5e-324, 1e-310, 0.0, -0.0, -1.0, np.inf, -np.inf,
                       np.nan])


def _structured():
    rng = np.random.default_rng(20240517)
    out = []
    for k in LOG_KS:
        for i in range(128):
            hw = interval_hi_word(i, k)
            if hw < 0x00100000 or hw + 0x2000 > 0x7FF00000:        # the interval leaves the positive normal range
                continue
            b0, b1 = hw << 32, ((hw + 0x2000) << 32) - 1
            pick = [b0, b0 + 1, b1 - 1, b1, (b0 + b1) // 2] + [int(v) for v in rng.integers(b0, b1 + 1, 16)]
            out.extend(from_bits(b) for b in pick)
    return np.array(out)


def _under_binade():
    """ln x just under 2^j: the result lies one binade below w = k ln2_hi + logc."""
    rng = np.random.default_rng(20240518)
    out = []
    for j in (-1, 0, 1, 2, 3):
        e = float(np.exp(np.float64(2.0 ** j)))
        b_lo, b_e = bits_of(e * (1 - 0.004)), bits_of(e)
        out.extend(from_bits(int(v)) for v in rng.integers(b_lo, b_e, 2000))
        out.extend(from_bits(b) for b in range(b_e - 64, b_e + 65))
    return np.array(out)


def _near_one():
    out = [1.0 + s * n * 2.0 ** -53 for n in range(65) for s in (1, -1)]
    for k in (0, 1):
        for i in (79, 80, 81):                                     # both edges of intervals 79 and 80
            e = bits_of(interval_ends(i, k)[0])
            out.extend(from_bits(b) for b in (e - 2, e - 1, e, e + 1))
    out.extend(neighbours(np.sqrt(0.5), 2))                        # the fdlibm reduction changes k here
    return np.array(out)


def _random_fifth():
    """The three random populations of test_hip_parity.py::test_device_log_accuracy at a fifth of their size."""
    rng = np.random.default_rng(11)
    return (rng.uniform(1e-4, 1.1e5, 40000), np.exp(rng.uniform(-700, 700, 20000)), 1.0 + rng.uniform(-1e-3, 1e-3, 10000))


@functools.lru_cache(maxsize=None)
def log_populations():
    """name -> arguments (read-only float64 arrays).  Every one but 'limits' holds positive normal doubles only."""
    pressures, magnitudes, near_one_random = _random_fifth()
    pops = {'structured': _structured(), 'under_binade': _under_binade(), 'near_one': _near_one(), 'limits': LOG_LIMITS.copy(),
            'pressures': pressures, 'magnitudes': magnitudes, 'near_one_random': near_one_random}
    for name, v in pops.items():
        assert v.dtype == np.float64 and v.size <= 100000, name
        v.setflags(write=False)
    return pops


@functools.lru_cache(maxsize=None)
def log_reference(name):
    """Exact ln of log_populations()[name]."""
    return exact_log(log_populations()[name])


@functools.lru_cache(maxsize=None)
def log_tab_reference(name):
    """log_tab_restated over log_populations()[name]: (value, defined, w) - value and w are NaN where not restated."""
    x = log_populations()[name]
    val, w = np.full(x.size, np.nan), np.full(x.size, np.nan)
    ok = np.zeros(x.size, dtype=bool)
    for j, v in enumerate(x):
        y, ww = log_tab_restated(v)
        if y is not NOT_RESTATED:
            val[j], w[j], ok[j] = y, ww, True
    for a in (val, w, ok):
        a.setflags(write=False)
    return val, ok, w


# ------------------------------------------------------------------ the float64 humidity chain
T0, TI = 273.16, 250.16
ESAT_LIMITS = (273.16, 250.16, 40.0, 32.19, -0.7, 0.0)
T_SPECIALS = np.array([-40.0, 1e-300, 1e20, 9.969209968386869e36, 1e300, np.inf, -np.inf, np.nan])
HUS_EDGES = np.array([0.0, -0.0, 1e-30, 1e-7, 3e-6, 0.03, 0.5, 1.0, np.nan])
PA_EDGES = np.array([1e-4, 1.0, 3e4, 101325.0, 1.1e5, 0.0, np.nan])
HUR_EDGES = np.array([0.0, 1e-3, 50.0, 100.0, 150.0, -5.0, np.nan])


@functools.lru_cache(maxsize=None)
def edge_temperatures():
    """(edges, sweeps): every limit of the e_sat paths with its four neighbours on each side and the special values; three
    seeded sweeps (mixed phase and its borders, the physical range, the unphysically cold range)."""
    rng = np.random.default_rng(20240519)
    edges = np.concatenate([neighbours(L, 4) for L in ESAT_LIMITS] + [T_SPECIALS])
    sweeps = np.concatenate([rng.uniform(249, 275, 4096), rng.uniform(40, 340, 4096), rng.uniform(-50, 70, 1024)])
    edges.setflags(write=False)
    sweeps.setflags(write=False)
    return edges, sweeps


def temperatures(dtype=np.float64):
    """The whole list, edges first; rounded to float32 for the float32-storage form."""
    with np.errstate(over='ignore'):
        return np.concatenate(edge_temperatures()).astype(dtype)


def humidity_operands(first, dtype=np.float64):
    """(x, pa, ta) for the three-operand wrappers: x cycles through `first` (HUS_EDGES, HUR_EDGES or one value of them), pa
    through PA_EDGES, such that every edge temperature meets every (x, pa) pair (a full product on the ~60 edge
    temperatures only) and the sweep temperatures go through the pairs one after another."""
    edges, sweeps = edge_temperatures()
    first = np.atleast_1d(np.asarray(first, dtype=np.float64))
    nx, npa = len(first), len(PA_EDGES)
    ta = np.concatenate([np.repeat(edges, nx * npa), sweeps])
    c = np.arange(ta.size)
    # any nx * npa consecutive c give every pair: by the Chinese remainder theorem where the lengths are coprime, by the
    # quotient and the remainder where they are not
    x = first[c % nx] if np.gcd(nx, npa) == 1 else first[(c // npa) % nx]
    pa = PA_EDGES[c % npa]
    with np.errstate(over='ignore'):
        return x.astype(dtype), pa.astype(dtype), ta.astype(dtype)


@functools.lru_cache(maxsize=None)
def hur_seeded():
    """509 seeded relative humidities in (-50, 200) for div_by_100 (509 is prime: the cycle through them and the one
    through the 7 pressures meet in every pair)."""
    v = np.random.default_rng(20240521).uniform(-50, 200, 509)
    v.setflags(write=False)
    return v


def shared_divisor_divide(n, d, r):
    """SharedDivisor::divide of pgw_device.h for finite doubles: q = n r, then fma(fma(-d, q, n), r, q)."""
    q = n * r
    return fma(fma(-d, q, n), r, q)


def alpha_literal(ta):
    """alpha of reference functions.py:91-105 as written there, in numpy."""
    alpha = np.full_like(ta, np.nan)
    alpha = np.where(ta >= T0, 1, alpha)
    alpha = np.where(ta <= TI, 0, alpha)
    with np.errstate(all='ignore'):
        alpha = np.where((ta < T0) & (ta > TI), np.power((ta - TI) / (T0 - TI), 2.), alpha)
    return alpha


def esat_argument(ta, water):
    """a3 (T - T0) / (T - a4) of reference functions.py:74-89 in numpy float64."""
    a3, a4 = (17.502, 32.19) if water else (22.587, -0.7)
    with np.errstate(all='ignore'):
        return a3 * (ta - T0) / (ta - a4)


@functools.lru_cache(maxsize=None)
def esat_reference(water):
    """Exact 611.21 * exp(esat_argument) over temperatures() (float64)."""
    return exact_exp(esat_argument(temperatures(), water), 611.21)


@functools.lru_cache(maxsize=None)
def esat_exp_is_normal(water):
    """Where exp(esat_argument) itself is a normal double (e_sat = 611.21 exp(..) is one for arguments 6.4 lower still)."""
    return exact_exp(esat_argument(temperatures(), water)).normal()


EXP_SPECIALS = np.array([0.0, -0.0, 1.0, -1.0, 709.78, 709.79, 710.0, 1024.0, 1025.0, -745.0, -745.2, -1075.0, -1076.0,
                         np.inf, -np.inf, np.nan, 1e-300, -1e-300, 5e-324])


EXP_GROUPS = ('esat_arguments', 'specials', 'sweep')


@functools.lru_cache(maxsize=None)
def _exp_groups():
    rng = np.random.default_rng(20240520)
    t = temperatures()
    return (np.concatenate([esat_argument(t, True), esat_argument(t, False)]), EXP_SPECIALS, rng.uniform(-760, 720, 50000))


@functools.lru_cache(maxsize=None)
def exp_arguments():
    """The e_sat arguments of the whole temperature list (both phases), the specials of test_device_exp_is_library_exp and
    50 000 seeded arguments in (-760, 720), in the order of EXP_GROUPS."""
    x = np.concatenate(_exp_groups())
    x.setflags(write=False)
    return x


def exp_group(name):
    """The slice of exp_arguments() that holds the group `name` of EXP_GROUPS."""
    sizes = [g.size for g in _exp_groups()]
    j = EXP_GROUPS.index(name)
    return slice(sum(sizes[:j]), sum(sizes[:j + 1]))


@functools.lru_cache(maxsize=None)
def exp_reference():
    return exact_exp(exp_arguments())


# ------------------------------------------------------------------ the table as tools/gen_log_table.py writes it
_FIX = 256                                   # fixed-point bits of the search below; the choice needs ~85


def _fixed(x):
    """The double x as an integer multiple of 2^-_FIX (exact)."""
    n, d = float(x).as_integer_ratio()
    return (n << _FIX) // d                  # d is a power of two below 2^_FIX for every value used here


@functools.lru_cache(maxsize=None)
def generated_log_table_header():
    """The text of pgw_log_table.h as tools/gen_log_table.py produces it, by the generator's own search - per interval the
    4097 doubles around 1 / centre, the one whose -ln lies closest to a double - in integer fixed-point arithmetic instead
    of 60-digit decimals (a second instead of half a minute): ln(base + j ulp) = ln(base) + log1p(j ulp / base) with
    ln(base) from mpmath and four terms of the series (the fifth is below 2^-200)."""
    one = 1 << _FIX
    rows, worst = [], 0
    for i in range(128):
        lo, hi = from_bits(interval_hi_word(i) << 32), from_bits((interval_hi_word(i) + 0x2000) << 32)
        with mp.workprec(_FIX + 64):
            base = float(1 / ((mpf(lo) + mpf(hi)) / 2))
            ln_base = int(mp.floor(mp.ldexp(mp.log(mpf(base)), _FIX) + mpf(0.5)))
        ulp = 2.0 ** -53 if base < 1 else 2.0 ** -52
        fb, fu = _fixed(base), _fixed(ulp)
        best = None
        for j in range(-2048, 2049):
            t = (j * fu << _FIX) // fb                             # j ulp / base
            t2 = t * t >> _FIX
            t3 = t2 * t >> _FIX
            exact = -(ln_base + t - t2 // 2 + t3 // 3 - (t2 * t2 >> _FIX) // 4)
            logc = exact / one                                     # int / int: the correctly rounded double
            err = abs(_fixed(logc) - exact)
            if best is None or err < best[0]:
                best = (err, base + j * ulp, logc)
        err, invc, logc = best
        if lo <= 1.0 < hi:
            invc, logc, err = 1.0, 0.0, 0
        worst = max(worst, err)
        rows.append((invc, logc, lo, hi))
    rmax = max(max(abs(lo * invc - 1), abs(hi * invc - 1)) for invc, logc, lo, hi in rows)
    out = ['// generated by tools/gen_log_table.py - do not edit.  {invc, logc} per interval of z in [0.6875, 1.375);\n',
           '// max |logc + log(invc)| = %.3e, max |r| = %.6f\n' % (worst / one, rmax),
           '#ifndef PGW_LOG_TABLE_BODY\n#ifndef PGW_LOG_TABLE_N_DEFINED\n#define PGW_LOG_TABLE_N_DEFINED\n'
           'namespace pgw { constexpr int LOG_TABLE_N = %d; }\n#endif\n#else\n' % 128]
    out += ['    %s, %s,\n' % (float.hex(invc), float.hex(logc)) for invc, logc, lo, hi in rows]
    out.append('#endif\n')
    return ''.join(out)
