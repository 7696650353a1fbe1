"""Host-side checks of the surface-pressure loop's control flow (pgw4era5_amd/csrc/pgw_loop_control.h): the reference's
stopping rule, the launch plan of the multi-pass kernel and the vector the latitude bands exchange.  A stand-alone C++
program that includes only that header runs scripted cases; what it must print comes from a Python transcription of
step_03_apply_to_era.py:186-189, 308-319 and of the plan / layout as DESIGN.md states them.  No GPU, no library."""
import math
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'pgw4era5_amd', 'csrc')
MAX_PASS = 8                 # passes of one launch at most (MULTI_MAX_PASS)
GUARD = 4                    # sentinel entries behind the history: nothing may be written there
SENTINEL = -777.0
INF, NAN = math.inf, math.nan

PROGRAM = r'''
#include <stdio.h>
#include <stdlib.h>
#include "pgw_loop_control.h"
using namespace pgw;

static const int GUARD = %d;
static const char *NAMES[] = {"CONTINUE", "CONVERGED", "NOT_CONVERGED"};
static char *cur;
static double num() { return strtod(cur, &cur); }
static void put(double x) { if (x != x) printf(" nan"); else printf(" %%.17g", x); }

// thresh max_n_iter hist_len planned guess n e1 .. en: the errors go to record() until it stops; planned = 1: launch by
// launch as the multi-pass loop does (the passes of a launch after the deciding one are speculation and are not recorded)
static void loop() {
    const double thresh = num();
    const int max_n_iter = (int)num(), hist_len = (int)num(), planned = (int)num(), guess = (int)num(), n = (int)num();
    double *errs = new double[n > 0 ? n : 1];
    for (int i = 0; i < n; ++i) errs[i] = num();
    double *hist = new double[hist_len + GUARD];
    for (int i = 0; i < hist_len + GUARD; ++i) hist[i] = %r;
    LoopControl lc{thresh, max_n_iter, 1, hist, hist_len};
    LoopControl::Verdict v = LoopControl::CONTINUE;
    int fed = 0, launched = 0;
    bool first = true;
    printf("launches");
    while (v == LoopControl::CONTINUE && fed < n) {
        const int allowed = lc.allowed();
        const int np = planned ? launch_passes(first, guess, max_n_iter, allowed) : 1;
        if (planned) printf(" %%d:%%d", np, allowed);
        launched += np;
        for (int k = 0; k < np && v == LoopControl::CONTINUE && fed < n; ++k) v = lc.record(errs[fed++]);
        first = false;
    }
    printf(" verdict %%s n_iter %%d it %%d launched %%d hist", NAMES[v], lc.n_iter(), lc.it, launched);
    for (int i = 0; i < hist_len + GUARD; ++i) put(hist[i]);
    printf("\n");
    delete[] errs;
    delete[] hist;
}

static void show(const BandVector &b, int np) {
    printf("length %%d raw", BandVector::length(np));
    for (int i = 0; i < BandVector::length(np); ++i) put(b.v[i]);
    printf(" pre %%d", b.pre());
    for (int k = 0; k < np; ++k) { printf(" pass %%d", b.code(k)); put(b.err(k)); }
    printf("\n");
}

// np pre, then per pass: code valid max
static void fill(BandVector &b, int np) {
    b.set_pre((int)num());
    for (int k = 0; k < np; ++k) {
        const int code = (int)num(), valid = (int)num();
        const double mx = num();
        b.set(k, code, valid != 0, mx);
    }
}

// np where code: the vector of a band that failed on its own, where = 0: before any reduce, 1: afterwards
static void failing(BandVector &b, int np) {
    const int where = (int)num(), code = (int)num();
    b.blank(np);
    if (where == 0) b.set_pre(code); else b.set(0, code, false, -INFINITY);
}

int main() {
    static char line[1 << 16];
    while (fgets(line, sizeof(line), stdin)) {
        cur = line + 1;
        BandVector a, b;
        int np;
        switch (line[0]) {
            case 'L': loop(); break;
            case 'V': np = (int)num(); fill(a, np); show(a, np); break;
            case 'B': np = (int)num(); failing(a, np); show(a, np); break;
            case 'M':               // MAX over two bands: a real vector and a failing one
                np = (int)num(); failing(b, np); fill(a, np);
                for (int i = 0; i < BandVector::length(np); ++i) a.v[i] = a.v[i] > b.v[i] ? a.v[i] : b.v[i];
                show(a, np);
                break;
            default: return 2;
        }
    }
    return 0;
}
''' % (GUARD, SENTINEL)


@pytest.fixture(scope='module')
def program(tmp_path_factory):
    """The compiled program and whether the sanitizers are in it (a compiler without their runtimes: a plain build)."""
    d = tmp_path_factory.mktemp('loop_control')
    src, exe = d / 'loop_control.cpp', d / 'loop_control'
    src.write_text(PROGRAM)
    cmd = [os.environ.get('CXX', 'c++'), '-std=c++17', '-Wall', '-I', CSRC, str(src), '-o', str(exe)]
    san = ['-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=undefined']
    sanitized = subprocess.call(cmd + san, stderr=subprocess.DEVNULL) == 0
    if not sanitized:
        subprocess.check_call(cmd)
    return str(exe), sanitized


def run(program, lines):
    out = subprocess.run([program[0]], input=''.join(s + '\n' for s in lines).encode(), stdout=subprocess.PIPE,
                         stderr=subprocess.PIPE)
    assert out.returncode == 0, out.stderr.decode()
    got = out.stdout.decode().splitlines()
    assert len(got) == len(lines)
    return [g.split() for g in got]


def fmt(x):
    return repr(float(x))


def same(a, b):
    return (a != a and b != b) or a == b


# ------------------------------------------------------------------ the transcriptions
def reference_loop(errs, thresh, max_n_iter):
    """step_03_apply_to_era.py:186-189, 308-319 with the passes' max |err| scripted: (raised, passes run, their errors)."""
    errs = iter(errs)
    seen = []
    phi_ref_max_error = INF                                     # :186
    it = 1                                                      # :188
    while phi_ref_max_error > thresh:                           # :189
        phi_ref_max_error = next(errs)                          # :308
        seen.append(phi_ref_max_error)
        it += 1                                                 # :313
        if it > max_n_iter:                                     # :315-319
            return True, it - 1, seen
    return False, it - 1, seen


def plan_launches(guess, max_n_iter, n_iter):
    """Passes of each launch of a file whose loop runs n_iter passes: the first launch carries the guess, clamped to
    [1, min(MAX_PASS, max_n_iter)], every later one 2; none more than max_n_iter still allows, none fewer than 1."""
    out, done = [], 0
    while done < n_iter:
        np_ = min(max(min(guess, MAX_PASS, max_n_iter), 1), max_n_iter - done) if not out else min(2, max_n_iter - done)
        out.append(max(np_, 1))
        done += out[-1]
    return out


def loop_line(errs, thresh, max_n_iter, hist_len, guess=None):
    return 'L %s %d %d %d %d %d %s' % (fmt(thresh), max_n_iter, hist_len, guess is not None, guess or 0, len(errs),
                                       ' '.join(fmt(e) for e in errs))


def check_loop(got, errs, thresh, max_n_iter, hist_len, guess=None):
    raised, n_iter, seen = reference_loop(errs, thresh, max_n_iter)
    i = got.index('verdict')
    assert got[i + 1] == ('NOT_CONVERGED' if raised else 'CONVERGED')
    assert int(got[i + 3]) == n_iter and int(got[i + 5]) == n_iter + 1
    hist = [float(x) for x in got[got.index('hist') + 1:]]
    want = (seen + [SENTINEL] * hist_len)[:hist_len] + [SENTINEL] * GUARD
    assert len(hist) == len(want) and all(same(h, w) for h, w in zip(hist, want)), (hist, want)
    if guess is not None:
        launches = [tuple(int(x) for x in s.split(':')) for s in got[1:i]]
        assert [np_ for np_, _ in launches] == plan_launches(guess, max_n_iter, n_iter)
        assert all(1 <= np_ and (np_ <= allowed or allowed < 1) for np_, allowed in launches)
        assert int(got[i + 7]) == sum(np_ for np_, _ in launches)              # passes_launched
    return n_iter


def tail(n, last=0.5):
    """n passes: n - 1 above the threshold 1.0, then `last`; 8 more follow for the passes a launch speculates"""
    return [9.0 - 0.01 * i for i in range(n - 1)] + [last] + [0.25] * 8


STOP_CASES = {
    'converges at pass 1': (tail(1), 1.0, 100, 32),
    'converges at pass 6, max_n_iter 7': (tail(6), 1.0, 7, 32),
    'converges at pass 6, max_n_iter 6: raised': (tail(6), 1.0, 6, 32),
    'NaN at pass 1': (tail(1, NAN), 1.0, 100, 32),
    'NaN at pass 4 of more': (tail(4, NAN), 1.0, 100, 32),
    'err == thresh': (tail(3, 1.0), 1.0, 100, 32),
    '+inf goes on': ([INF, INF] + tail(2), 1.0, 100, 32),
    'max_n_iter 1, converged': (tail(1), 1.0, 1, 32),
    'max_n_iter 1, not converged': (tail(3), 1.0, 1, 32),
    'max_n_iter 0': (tail(2), 1.0, 0, 32),
    '40 passes, 32 entries': (tail(40), 1.0, 100, 32),
    '40 passes, raised at 40': (tail(40), 1.0, 40, 32),
    'history as long as max_n_iter': (tail(5), 1.0, 5, 5),
    'no history': (tail(3), 1.0, 100, 0),
}


def test_sanitizers_are_in_the_program(program):
    if not program[1]:
        pytest.skip('the host compiler has no AddressSanitizer / UBSan runtime: the program of this module is a plain build')


def test_the_transcription_itself():
    assert reference_loop(tail(6), 1.0, 7) == (False, 6, tail(6)[:6])
    assert reference_loop(tail(6), 1.0, 6)[:2] == (True, 6)
    assert reference_loop([5.0, NAN, 0.0], 1.0, 9)[:2] == (False, 2)
    assert plan_launches(6, 100, 6) == [6] and plan_launches(5, 100, 6) == [5, 2] and plan_launches(8, 100, 6) == [8]
    assert plan_launches(1, 100, 6) == [1, 2, 2, 2] and plan_launches(6, 7, 7) == [6, 1]


@pytest.mark.parametrize('name', list(STOP_CASES))
def test_stopping_rule(program, name):
    """One launch per pass (the per-pass loop and the re-interpolating file loop) and the same errors through the plan."""
    errs, thresh, max_n_iter, hist_len = STOP_CASES[name]
    single, planned = run(program, [loop_line(errs, thresh, max_n_iter, hist_len),
                                    loop_line(errs, thresh, max_n_iter, hist_len, guess=6)])
    n = check_loop(single, errs, thresh, max_n_iter, hist_len)
    assert n == check_loop(planned, errs, thresh, max_n_iter, hist_len, guess=6)
    want = {'converges at pass 1': 1, 'converges at pass 6, max_n_iter 7': 6, 'converges at pass 6, max_n_iter 6: raised': 6,
            'NaN at pass 1': 1, 'NaN at pass 4 of more': 4, 'err == thresh': 3, '+inf goes on': 4, '40 passes, 32 entries': 40}
    assert name not in want or n == want[name]


@pytest.mark.parametrize('max_n_iter', [1, 2, 3, 100])
def test_launch_plan(program, max_n_iter):
    guesses = [0, -3, 1, 2, 5, 8, 9, 1000]
    cases = [(g, c) for g in guesses for c in (1, 2, 3, 6, 7, 11) if c <= max_n_iter + 1]
    got = run(program, [loop_line(tail(c), 1.0, max_n_iter, 32, guess=g) for g, c in cases])
    for (g, c), line in zip(cases, got):
        assert check_loop(line, tail(c), 1.0, max_n_iter, 32, guess=g) == min(c, max(max_n_iter, 1))


def vec_line(kind, np_, pre, passes, head=''):
    return '%s %d %s%d %s' % (kind, np_, head, pre, ' '.join('%d %d %s' % (c, v, fmt(m)) for c, v, m in passes))


def parse_vec(got, np_):
    n = int(got[1])
    raw = [float(x) for x in got[3:3 + n]]
    rest = got[3 + n:]
    assert rest[0] == 'pre' and len(rest) == 2 + 3 * np_
    return n, raw, int(rest[1]), [(int(rest[3 + 3 * k]), float(rest[4 + 3 * k])) for k in range(np_)]


def flat(pre, passes):
    return [float(pre)] + [float(x) for c, v, m in passes for x in (c, v, m)]


@pytest.mark.parametrize('np_', [1, 2, 8])
def test_exchange_vector_round_trip(program, np_):
    passes = [(0, 1, 3.5 + k) for k in range(np_)]
    passes[-1] = (0, 0, -INF)                                                  # a pass without a valid column
    with_code = [(7, 1, 2.0)] + passes[1:]
    got = run(program, [vec_line('V', np_, 0, passes), vec_line('V', np_, 5, with_code)])
    for line, pre, ps in zip(got, (0, 5), (passes, with_code)):
        n, raw, got_pre, got_passes = parse_vec(line, np_)
        assert n == 1 + 3 * np_ and raw == flat(pre, ps) and got_pre == pre
        for (code, valid, mx), (got_code, got_err) in zip(ps, got_passes):
            assert got_code == code and same(got_err, mx if valid else NAN)


@pytest.mark.parametrize('np_', [1, 2, 8])
def test_exchange_vector_of_a_failing_band(program, np_):
    """The two vectors a band that stops on its own sends, and what the other bands read after the MAX with theirs."""
    nothing = [(0, 0, -INF)] * np_
    real = [(0, 1, 0.5 ** k) for k in range(np_)]                              # every pass below a threshold of 1.0 ...
    before, after, met_before, met_after = run(program, [
        'B %d 0 4' % np_, 'B %d 1 4' % np_, vec_line('M', np_, 0, real, head='0 4 '), vec_line('M', np_, 0, real, head='1 4 ')])
    assert parse_vec(before, np_)[:3] == (1 + 3 * np_, flat(4, nothing), 4)
    assert parse_vec(after, np_)[:2] == (1 + 3 * np_, flat(0, [(4, 0, -INF)] + nothing[1:]))
    # ... yet the status is what the loop reads first: slot by slot before any pass is recorded
    n, raw, pre, passes = parse_vec(met_before, np_)
    assert pre == 4 and raw == [max(a, b) for a, b in zip(flat(0, real), flat(4, nothing))]
    n, raw, pre, passes = parse_vec(met_after, np_)
    assert pre == 0 and passes[0][0] == 4 and raw == [max(a, b) for a, b in zip(flat(0, real), flat(0, [(4, 0, -INF)] + nothing[1:]))]
