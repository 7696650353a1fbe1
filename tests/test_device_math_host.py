"""CPU-side checks behind tests/test_device_math_hip.py: the logarithm table of pgw_log_tab, the exact restatement of
pgw_log_tab against the exact logarithm, and the checker itself (tests/device_math_cases.py).  No GPU."""
import math
import os
import sys
from fractions import Fraction

import numpy as np
import pytest
from mpmath import mp, mpf

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import device_math_cases as M                                                         # noqa: E402

# measured with the restatement (which the GPU test requires the device to equal bit for bit) over every population
MEASURED_MAX_ULP, MEASURED_MAX_AT = 1.4893, 1.6487212707001178


def test_log_table_is_what_its_header_and_pgw_device_h_say():
    """pgw_log_table.h: 128 {invc, logc} pairs written as exact doubles; the interval that starts at 1.0 (index 80; 79
    ends there) holds {1, 0}; |logc + ln(invc)| <= 2.2e-19 against the exact logarithm (the header's second line);
    |r| = |fma(z, invc, -1)| < 0.0040 at both ends of every interval but 79 and 80 (the bound pgw_device.h uses for the
    truncation term; those two go to the fdlibm kernel for k = 0 and reach |r| = 2^-7 otherwise).
    test_log_table_header_is_the_generators_output_byte_for_byte holds the file to the generator's output."""
    text, tab = M.log_table_text(), M.log_table()
    assert len(text) == 256 and len(tab) == 128
    for h in text:                                                 # every literal is a double: it survives the round trip
        assert float.hex(float.fromhex(h)) == h, h
    one = (M.bits_of(1.0) >> 32) - M.TAB_OFF_HI >> 13
    assert one == 80 and tab[80] == (1.0, 0.0) and M.interval_ends(80)[0] == 1.0 and M.interval_ends(79)[1] == np.nextafter(1.0, 0)
    with mp.workprec(M.PREC):
        worst = float(max(abs(mpf(logc) + mp.log(mpf(invc))) for invc, logc in tab))
    assert worst <= 2.2e-19, worst
    assert worst > 1e-19                                    # the figure the header prints (2.162e-19) is this one
    rmax = 0.0
    for i, (invc, logc) in enumerate(tab):
        ends = [abs(M.fma(z, invc, -1.0)) for z in M.interval_ends(i)]
        if i in (79, 80):
            assert max(ends) <= 2.0 ** -7
        else:
            rmax = max(rmax, *ends)
    assert 0.0035 < rmax < 0.0040, rmax


def test_log_table_header_is_the_generators_output_byte_for_byte():
    """pgw_log_table.h is what tools/gen_log_table.py writes, byte for byte: its two comment lines with the figures they
    print, the preprocessor frame, and all 128 pairs - per interval, among the 4097 doubles around 1 / centre, the invc whose
    -ln lies closest to a double, and that double as logc (interval 80: {1, 0}).  The generator itself can run from a
    scratch directory but takes half a minute in 60-digit decimals; device_math_cases.generated_log_table_header repeats
    its search in integer fixed-point arithmetic in under two seconds."""
    with open(os.path.join(M.CSRC, 'pgw_log_table.h')) as f:
        committed = f.read()
    assert M.generated_log_table_header() == committed


def test_restatement_takes_the_table_path_where_pgw_log_tab_does():
    """NOT_RESTATED exactly for arguments that are not positive normal finite doubles and for intervals 79 and 80 of k = 0,
    i.e. [1 - 2^-8, 1 + 2^-7)."""
    for name in ('limits', 'near_one', 'structured'):
        x = M.log_populations()[name]
        _, ok, _ = M.log_tab_reference(name)
        with np.errstate(invalid='ignore'):
            normal = (x >= M.MIN_NORMAL) & (x <= M.MAX_DOUBLE)
            want = normal & ~((x >= 1 - 2.0 ** -8) & (x < 1 + 2.0 ** -7))
        np.testing.assert_array_equal(ok, want, err_msg=name)
    assert M.log_tab_reference('structured')[1].sum() > 30000


@pytest.mark.parametrize('name', ['structured', 'under_binade', 'near_one', 'limits', 'pressures', 'magnitudes'])
def test_restated_log_tab_against_the_exact_logarithm(name):
    """pgw_log_tab's arithmetic (exact restatement) against the exact logarithm: <= 1.8 ulp, the derived bound - 0.5 from
    the final rounding, up to 1.0 from the uncompensated rounding of w = fma(k, ln2_hi, logc) where the result lies one
    binade below w, <= 0.25 from logc's 2.2e-19 against the smallest result ulp 2^-60, < 0.05 for the remaining
    roundings.  The result cannot lie two binades below w where w is rounded: for k = 0, w is logc itself (no rounding;
    |logc| goes down to 0.0059 in interval 78), and for k != 0, |w| >= ln 1.375 = 0.318 against |r| < 0.004 - asserted
    below.  Every argument above 1.0 ulp must show the mechanism: |w| in the binade above |result|.
    Measured: maximum 1.489 ulp at x = 1.6487212707001178 (population 'under_binade'; ln x = 0.4999999999999937 under
    w = 0.50219); 1.334 ulp at x = 1.6484375, the first double of an interval; above 1 ulp
    3 of 30 534 arguments of 'structured' and 197 of 10 645 of 'under_binade', all of them just under sqrt(e); 'near_one'
    0.74, 'limits' 0.79, 'pressures' 0.9986, 'magnitudes' 0.9999.  Not correctly rounded: 23 % of 'structured', 25 % of
    'pressures'.  ('near_one_random' lies wholly in intervals 79 and 80 of k = 0: nothing to restate.)"""
    x = M.log_populations()[name]
    val, ok, w = M.log_tab_reference(name)
    assert ok.any() and not M.log_tab_reference('near_one_random')[1].any()
    ref = M.log_reference(name)
    err = np.abs(ref.ulp_error(val))[ok]
    xs, ws, rd = x[ok], w[ok], ref.rd[ok]
    worst = int(np.argmax(err))
    print('%s: %d arguments, max %.4f ulp at %r, above 1 ulp: %d, not correctly rounded: %.3f %%'
          % (name, err.size, err[worst], xs[worst], (err > 1).sum(), 100 * (val[ok] != rd).mean()))
    assert err[worst] <= 1.8, (err[worst], xs[worst])
    assert err[worst] <= MEASURED_MAX_ULP + 0.0005, (err[worst], xs[worst])      # what the comment in pgw_device.h states
    over = err > 1.0
    assert (np.frexp(np.abs(ws[over]))[1] == np.frexp(np.abs(rd[over]))[1] + 1).all(), xs[over]
    k0 = (xs >= 0.6875) & (xs < 1.375)
    tab_logc = np.array([logc for _, logc in M.log_table()])
    assert np.isin(ws[k0], tab_logc).all() and (np.abs(ws[~k0]) >= 0.318).all()
    if name == 'under_binade':
        assert xs[worst] == MEASURED_MAX_AT and abs(err[worst] - MEASURED_MAX_ULP) < 0.0005
    if name == 'structured':                                       # the figure of the issue that asked for this test
        at = np.flatnonzero(xs == 1.6484375)
        assert at.size and abs(err[at[0]] - 1.334) < 0.0005


def test_what_the_seeded_hur_can_tell_of_the_reciprocal_of_100():
    """The power of the relative humidities of the GPU test of relative_to_specific_humidity over div_by_100 =
    SharedDivisor(100, 0.01).divide, restated with exact fmas.  With r = 0.01 every quotient is hur / 100.  The residual
    step absorbs an error of the reciprocal far beyond its last bit: one ulp off, and 2^20 ulps off, still give hur / 100
    for every value - a wrong last bit of r is not a fault that any numerator could show.  From a relative error of 2^-28
    (2^24 ulps) on, 23 of the 509 seeded values come out wrong and none of the seven of the edge list: the seeded ones are
    what holds div_by_100 to the division."""
    r, ulp = 0.01, float(np.spacing(0.01))
    seeded = M.hur_seeded().tolist()
    edges = [h for h in M.HUR_EDGES.tolist() if h == h]

    def wrong(values, rr):
        return sum(M.shared_divisor_divide(h, 100.0, rr) != h / 100 for h in values)
    assert wrong(seeded + edges, r) == 0
    for k in (1, 2 ** 20):
        assert wrong(seeded + edges, r + k * ulp) == 0 and wrong(seeded + edges, r - k * ulp) == 0
    for k in (2 ** 24, -2 ** 24):
        assert wrong(seeded, r + k * ulp) >= 10 and wrong(edges, r + k * ulp) == 0


def test_the_checker_checks_itself():
    """exact_log / exact_exp agree with math.log / math.exp to 1 ulp on 1000 points each, are exact at ln 1 = 0 and
    e^0 = 1, place a known error where it is (one ulp up is +1 minus the rounding residue), and the integer fma is
    float(Fraction(a) * Fraction(b) + Fraction(c))."""
    rng = np.random.default_rng(5)
    x = np.concatenate([np.exp(rng.uniform(-700, 700, 500)), rng.uniform(0.5, 2.0, 500)])
    ref = M.exact_log(x)
    assert np.abs(ref.ulp_error(np.array([math.log(v) for v in x]))).max() <= 1.0
    assert (np.abs(ref.rest) <= 0.5 * np.spacing(np.abs(ref.rd))).all()
    e = ref.ulp_error(np.nextafter(ref.rd, np.inf))
    assert (e > 0.49).all() and (e < 1.51).all()
    y = rng.uniform(-700, 700, 1000)
    refe = M.exact_exp(y)
    assert np.abs(refe.ulp_error(np.array([math.exp(v) for v in y]))).max() <= 1.0
    one = M.exact_log(np.array([1.0, 0.0, np.inf, -1.0, np.nan]))
    assert one.rd[0] == 0.0 and one.rest[0] == 0.0 and one.rd[1] == -np.inf and one.rd[2] == np.inf and np.isnan(one.rd[3:]).all()
    zero = M.exact_exp(np.array([0.0, 1.0, 800.0, -800.0, np.nan]))
    assert zero.rd[0] == 1.0 and zero.rest[0] == 0.0 and zero.rd[1] == math.e and zero.rd[2] == np.inf and zero.rd[3] == 0.0
    assert np.isnan(zero.rd[4])
    scaled = M.exact_exp(np.array([0.0]), 611.21)
    assert scaled.rd[0] == 611.21 and scaled.rest[0] == 0.0
    a, b = rng.uniform(-2, 2, 2000), rng.uniform(-2, 2, 2000)
    c = np.where(np.arange(2000) % 2 == 0, -(a * b), rng.uniform(-2, 2, 2000))      # half of them cancel: the residue of a product
    for u, v, t in zip(a.tolist(), b.tolist(), c.tolist()):
        assert M.fma(u, v, t) == float(Fraction(u) * Fraction(v) + Fraction(t))
    assert M.fma(3.0, 0.5, -1.5) == 0.0 and math.copysign(1.0, M.fma(-1.0, 0.0, -0.0)) == -1.0
