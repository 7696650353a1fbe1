"""PGW_OPT_FINISH_IN_PASS ('finish_in_pass'): the storing pass of the multi-pass loop kernel goes on from where its scan
stopped to the first hybrid level and writes PS, so a file whose predicted pass converges launches no finalize kernel, and
the surface riders are enqueued behind the first loop launch's status read-back instead of first.  The option changes who
writes a value and when, never the value: on (default) against off, in one process, every output has the same bits and the
loop runs the same passes.  `Context.last_qv_from_pass()` and the profiler's count of finalize launches say which way a
file went.

float32 files in reference-dtype mode take the riders' new place but not the longer pass (their loop launch lost about as much
as their finalize kernel gave: DESIGN.md section 4; excluded by template like float32 fast storage from 'qv_from_pass'): for them
the option must leave the finalize launch with its marks as it was, which is what FINISHES says.

Shapes: 20 model levels, 6 of them pure-pressure levels (or none), 5 delta levels, 300 columns (four full waves and one of
44 lanes) and 64; float64 files and float32 files in reference-dtype mode.  A file has one time step (two fail like the
reference, tests/test_hip_parity.py), so ntime = 2 runs through the function-level loop, `functions.adjust_ps_loop`, which
launches the same kernel with every level its own (no level written before the loop).

The host-only part runs pgw_loop_control.h's LoopControl, launch_passes and StoredPass in a stand-alone program against a
Python transcription of the rule: nothing is launched after the loop exactly when the pass the reference's stopping rule
chooses is the last pass of its launch, that launch stored and finished, and its maximum is a number."""
import math
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'pgw4era5_amd', 'csrc')
N_LEV, N_PURE = 20, 6
PLEV5 = np.array([100000.0, 85000.0, 30000.0, 2000.0, 500.0])
STORAGE = {'f64': (np.float64, False), 'f32ref': (np.float32, True)}
FINISHES = {'f64': True, 'f32ref': False}      # the storing pass of this storage walks on to the first hybrid level
OUTPUTS = ('PS', 'QV', 'T', 'U', 'V', 'T_SKIN', 'T_SO', 'FR_SEA_ICE')
MAX_PASS = 8


# ------------------------------------------------------------------ cases
def coefficients(n_pure):
    """ak, bk of synthetic.hybrid_coefficients(20) with the same half-level pressures at ps = 101325 Pa, but bk = 0 on half
    levels 0 .. n_pure (n_pure pure-pressure full levels; 0: bk > 0 from half level 1 on, every full level hybrid)."""
    n = N_LEV
    k = np.arange(n + 1, dtype=np.float64)
    p = 101325.0 * (k / n) ** (np.log(101325.0) / np.log(float(n)))
    s = np.clip((p - p[n_pure]) / (101325.0 - p[n_pure]), 0.0, 1.0)
    bk = s ** 1.6
    bk[-1] = 1.0
    ak = p - bk * 101325.0
    ak[-1] = ak[0] = 0.0
    bkm = 0.5 * (bk[1:] - bk[:-1]) + bk[:-1]
    assert int((bkm == 0.0).sum()) == n_pure and np.all(bkm[n_pure:] > 0.0)
    for ps in (50000.0, 105000.0):
        assert np.all(np.diff(ak + bk * ps) > 0.0)
    return ak, bk


def take_columns(c, idx):
    """The case cut to the flat columns `idx`, as a file of one latitude row."""
    def cut(v):
        if isinstance(v, np.ndarray) and v.ndim >= 3:
            return np.ascontiguousarray(v.reshape(v.shape[:-2] + (-1,))[..., idx][..., None, :])
        return v
    return dict(c, era={k: cut(v) for k, v in c['era'].items()}, deltas={k: cut(v) for k, v in c['deltas'].items()})


def make(ncol, dtype=np.float64, n_pure=N_PURE, flat=False, seed=3):
    """`ncol` columns of a synthetic file on the coefficients above, mountains included (surface 1013 .. 540 hPa) or, with
    `flat`, sea columns only (surface above 980 hPa: a reference level close to the ground lies above it everywhere)."""
    from pgw4era5_amd import synthetic
    c = synthetic.make_case(nlat=20, nlon=32, nlev=N_LEV, seed=seed, dtype=dtype, plev=PLEV5)
    ps = c['era']['PS'].reshape(-1).astype(np.float64)
    idx = np.nonzero(ps > 98000.0)[0] if flat else np.arange(ps.size)
    assert idx.size >= ncol
    c = take_columns(c, idx[:ncol])
    ak, bk = coefficients(n_pure)
    era = dict(c['era'], ak=ak, bk=bk)
    era.pop('akm', None), era.pop('bkm', None)
    return dict(c, era=era)


def both(c, ref, guess=None, opts=None, **kw):
    """The file with finish_in_pass = 1 and = 0, other options as given.  [(result or ValueError, (used, skipped),
    finalize launches), ...]"""
    from pgw4era5_amd import step_03_apply_to_era as s3
    from pgw4era5_amd.device import default_context
    ctx = default_context()
    old = {k: ctx.set_option(k, v) for k, v in dict(opts or {}).items()}
    old['finish_in_pass'] = ctx.get_option('finish_in_pass')
    old['loop_guess'] = ctx.get_option('loop_guess')
    res = []
    try:
        ctx.profile(True)
        for on in (1, 0):
            ctx.set_option('finish_in_pass', on)
            if guess is not None:
                ctx.set_option('loop_guess', guess)
            ctx.profile_reset()
            try:
                r = s3.pgw_for_era5_arrays(c['era'], c['deltas'], c['delta_times'], c['plev'], c['target_dt'], True,
                                           ref_dtype=ref, **kw)
            except ValueError as e:
                r = e
            res.append((r, ctx.last_qv_from_pass(), ctx.profile_get('finalize')[0]))
    finally:
        ctx.profile(False)
        for k, v in old.items():
            ctx.set_option(k, v)
    return res


def same_file(a, b):
    assert not isinstance(a, Exception) and not isinstance(b, Exception), (a, b)
    assert a['n_iter'] == b['n_iter'] and a['passes_launched'] == b['passes_launched']
    np.testing.assert_array_equal(np.asarray(a['max_err']), np.asarray(b['max_err']))
    for k in OUTPUTS:
        assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)            # NaN only where the other has NaN


def check(res, branch, hybrid_level_columns, finishes=True):
    """On and off give the same file; on took `branch` ('none': no launch after the loop, 'all': the finalize kernel over
    all levels, 'off': the loop did not store at all), off is the parent's sequence with one finalize launch.  A storage
    whose pass does not finish its columns (`finishes` false) keeps that sequence and its marks with the option on."""
    (a, ma, fa), (b, mb, fb) = res
    same_file(a, b)
    assert fb == 1
    if branch == 'none' and not finishes:
        assert ma == mb and fa == 1
        assert mb[0] and 0 < mb[1] <= hybrid_level_columns
    elif branch == 'none':
        assert ma == (True, hybrid_level_columns) and fa == 0
        assert mb[0] and 0 < mb[1] <= hybrid_level_columns             # the marks of the same pass, used by the kernel
    else:
        assert ma == (False, 0) and fa == 1 and mb == (False, 0)
    return a


def n_iter_of(c, ref, **kw):
    r = both(c, ref, **kw)[0][0]
    assert not isinstance(r, Exception), r
    return r['n_iter']


pytestmark_gpu = pytest.mark.gpu


# ------------------------------------------------------------------ GPU: files
@pytestmark_gpu
def test_option_defaults_to_on():
    from pgw4era5_amd.device import default_context
    assert default_context().get_option('finish_in_pass') == 1


@pytestmark_gpu
@pytest.mark.parametrize('ncol', [300, 64])
@pytest.mark.parametrize('storage', sorted(STORAGE))
def test_branches_of_the_prediction(storage, ncol):
    """1. the predicted pass converges: no launch after the loop.  2. convergence one pass earlier than the stored one: the
    finalize kernel overwrites what was speculated.  3. a first launch two passes short: the continuation launch's last
    pass finishes the columns; one pass short: its first pass converges, its second stored - the finalize kernel again."""
    dtype, ref = STORAGE[storage]
    c = make(ncol, dtype)
    ps = c['era']['PS']
    assert ps.min() < 80000.0 and ps.max() > 100000.0                   # waves that pass p_ref at different levels
    n = n_iter_of(c, ref)
    assert 3 <= n < MAX_PASS
    hyb = ncol * (N_LEV - N_PURE)
    for guess, branch in ((n, 'none'), (n + 1, 'all'), (n - 2, 'none'), (n - 1, 'all')):
        a = check(both(c, ref, guess), branch, hyb, FINISHES[storage])
        assert a['n_iter'] == n


@pytestmark_gpu
@pytest.mark.parametrize('storage', sorted(STORAGE))
def test_unfused_first_launch(storage):
    """fused_first = 0: one kernel runs all passes of the first launch, the ERA-state scan included."""
    dtype, ref = STORAGE[storage]
    c = make(300, dtype)
    n = n_iter_of(c, ref, opts=dict(fused_first=0))
    check(both(c, ref, n, dict(fused_first=0)), 'none', 300 * (N_LEV - N_PURE), FINISHES[storage])
    check(both(c, ref, n + 1, dict(fused_first=0)), 'all', 300 * (N_LEV - N_PURE), FINISHES[storage])


@pytestmark_gpu
@pytest.mark.parametrize('storage', sorted(STORAGE))
def test_all_levels_hybrid_and_full_column(storage):
    """4. n_pure = 0: the storing pass walks to level 0.  full_column = 1: one launch per pass, the option has nothing to
    act on (and the riders stay first)."""
    dtype, ref = STORAGE[storage]
    c = make(300, dtype, n_pure=0)
    n = n_iter_of(c, ref)
    check(both(c, ref, n), 'none', 300 * N_LEV, FINISHES[storage])
    check(both(c, ref, n, dict(full_column=1)), 'off', 300 * N_LEV, FINISHES[storage])
    check(both(make(64, dtype), ref, n, dict(multipass=0)), 'off', 0, FINISHES[storage])


def bend_one_layer(c, ps_turn):
    """ak altered at one half level so that the layer above it has zero thickness at ps = ps_turn and a negative one below:
    ps_mono_min becomes ps_turn (as tests/test_qv_from_pass.py does)."""
    era = dict(c['era'])
    ak, bk = era['ak'].copy(), era['bk'].copy()
    l = len(ak) - 6
    assert bk[l + 1] > bk[l]
    ak[l + 1] = ak[l] - ps_turn * (bk[l + 1] - bk[l])
    era['ak'] = ak
    return dict(c, era=era)


@pytestmark_gpu
@pytest.mark.parametrize('storage', sorted(STORAGE))
def test_columns_that_never_vote_to_stop(storage):
    """5. ps below ps_mono_min in some columns, each in a wave with ordinary ones: those waves walk to the top, their
    extension is empty, the others' is not.  And a NaN ps: the file raises the same error either way."""
    dtype, ref = STORAGE[storage]
    c = bend_one_layer(make(300, dtype), 75000.0)
    ps = c['era']['PS'].reshape(-1)
    low = np.array([(ps[i:i + 64] < 75000.0).any() for i in range(0, ps.size, 64)])
    mixed = np.array([0 < (ps[i:i + 64] < 75000.0).sum() < len(ps[i:i + 64]) for i in range(0, ps.size, 64)])
    assert low.any() and not low.all() and mixed.any()
    n = n_iter_of(c, ref)
    check(both(c, ref, n), 'none', 300 * (N_LEV - N_PURE), FINISHES[storage])
    c = make(300, dtype)
    era = dict(c['era'])
    era['PS'] = c['era']['PS'].copy()
    era['PS'][0, 0, 70] = np.nan
    (a, ma, _), (b, mb, _) = both(dict(c, era=era), ref, 6)
    assert isinstance(a, ValueError) and isinstance(b, ValueError), (a, b)
    assert str(a) == str(b) and getattr(a, 'column', None) == getattr(b, 'column', None) == 70
    assert ma == (False, 0) and mb == (False, 0)


@pytestmark_gpu
@pytest.mark.parametrize('storage', sorted(STORAGE))
def test_reference_level_at_both_ends(storage):
    """6. p_ref = 20 hPa: half level 8 lies at or below it everywhere, so every wave's scan (two levels a step) ends on
    level 6, the first hybrid level - the extension is empty.  p_ref = 850 hPa over sea columns: half level 18 lies
    above it, the scan stops after levels 19 and 18 and the extension walks the other twelve hybrid levels."""
    dtype, ref = STORAGE[storage]
    c = make(300, dtype)
    ak, bk = c['era']['ak'], c['era']['bk']
    assert (ak[8] + bk[8] * c['era']['PS'].astype(np.float64)).min() >= 2000.0
    n = n_iter_of(c, ref, p_ref=2000.0)
    (a, ma, _), (b, mb, _) = res = both(c, ref, n, p_ref=2000.0)
    check(res, 'none', 300 * (N_LEV - N_PURE), FINISHES[storage])
    assert mb == (True, 300 * (N_LEV - N_PURE))                         # the scan alone got there
    c = make(300, dtype, flat=True)
    assert (ak[18] + bk[18] * c['era']['PS'].astype(np.float64)).max() < 85000.0 < c['era']['PS'].min()
    n = n_iter_of(c, ref, p_ref=85000.0)
    (a, ma, _), (b, mb, _) = res = both(c, ref, n, p_ref=85000.0)
    check(res, 'none', 300 * (N_LEV - N_PURE), FINISHES[storage])
    assert mb == (True, 300 * 2)


# ------------------------------------------------------------------ GPU: the loop on its own, ntime = 1 and 2
@pytestmark_gpu
@pytest.mark.parametrize('ncol', [300, 64])
@pytest.mark.parametrize('ntime', [1, 2])
def test_function_level_loop(ntime, ncol):
    """functions.adjust_ps_loop (every level is the loop's: l_start = 0), one and two time steps: PS and QV of both time
    steps have the same bits, predicted exactly (nothing launched) and one pass long (finalize over all levels)."""
    from oracle import pgw_oracle as O
    from pgw4era5_amd import functions as F
    from pgw4era5_amd.device import default_context
    ctx = default_context()
    cs = [make(ncol, seed=3 + t) for t in range(ntime)]
    era = {k: (np.concatenate([c['era'][k] for c in cs], axis=0) if isinstance(v, np.ndarray) and v.ndim >= 3 else v)
           for k, v in cs[0]['era'].items()}
    _, pa = O.hybrid_pressure(era['ak'], era['bk'], era['PS'])
    hur = O.specific_to_relative_humidity(era['QV'], pa, era['T'])
    dzg = np.concatenate([c['deltas']['zg'][6, 2][None] for c in cs], axis=0)           # the record at p_ref = 300 hPa

    def run(on, guess):
        old = ctx.set_option('finish_in_pass', on), ctx.get_option('loop_guess')
        try:
            if guess is not None:
                ctx.set_option('loop_guess', guess)
            ctx.profile(True)
            ctx.profile_reset()
            r = F.adjust_ps_loop(era['ak'], era['bk'], era['PS'], era['FIS'], era['T'], era['QV'], era['T'] + 2.0, hur - 1.0,
                                 dzg, p_ref=30000.0)
            return r, ctx.last_qv_from_pass(), ctx.profile_get('finalize')[0]
        finally:
            ctx.profile(False)
            ctx.set_option('finish_in_pass', old[0])
            ctx.set_option('loop_guess', old[1])

    n = run(1, None)[0]['n_iter']
    assert 2 <= n < MAX_PASS
    for guess, nothing in ((n, True), (n + 1, False)):
        (a, ma, fa), (b, mb, fb) = run(1, guess), run(0, guess)
        assert a['n_iter'] == b['n_iter'] == n and a['max_err'] == b['max_err']
        np.testing.assert_array_equal(a['ps_pgw'], b['ps_pgw'])
        np.testing.assert_array_equal(a['hus_pgw'], b['hus_pgw'])
        assert a['ps_pgw'].shape[0] == ntime
        assert fb == 1 and fa == (0 if nothing else 1)
        assert ma == ((True, ntime * ncol * N_LEV) if nothing else (False, 0))
        assert mb[0] == nothing


# ------------------------------------------------------------------ host only: the launch decision
PROGRAM = r'''
#include <stdio.h>
#include <stdlib.h>
#include "pgw_loop_control.h"
using namespace pgw;

static const char *FINAL[] = {"NOTHING", "ABOVE_MARKS", "ALL_LEVELS"};
static const char *VERDICT[] = {"CONTINUE", "CONVERGED", "NOT_CONVERGED"};

// thresh max_n_iter guess fused stores finish n e1 .. en: launch by launch as the multi-pass loop goes - the last pass of a
// launch stores (with `fused`, a first launch of one pass is the flagged kernel alone, which does not), the recorded
// maxima go to LoopControl::record until it stops, the pass it chooses to StoredPass::decided
int main() {
    static char line[1 << 16];
    while (fgets(line, sizeof(line), stdin)) {
        char *cur = line;
        const double thresh = strtod(cur, &cur);
        const int max_n_iter = (int)strtod(cur, &cur), guess = (int)strtod(cur, &cur), fused = (int)strtod(cur, &cur);
        const int stores = (int)strtod(cur, &cur), finish = (int)strtod(cur, &cur), n = (int)strtod(cur, &cur);
        double *errs = new double[n > 0 ? n : 1];
        for (int i = 0; i < n; ++i) errs[i] = strtod(cur, &cur);
        LoopControl lc{thresh, max_n_iter};
        LoopControl::Verdict v = LoopControl::CONTINUE;
        StoredPass sp;
        bool first = true;
        int fed = 0;
        while (v == LoopControl::CONTINUE && fed < n) {
            const int np = launch_passes(first, guess, max_n_iter, lc.allowed());
            sp.launched(stores && !(first && fused && np == 1) ? np - 1 : -1, finish != 0);
            for (int k = 0; k < np && v == LoopControl::CONTINUE && fed < n; ++k) {
                const double e = errs[fed++];
                v = lc.record(e);
                if (v == LoopControl::CONVERGED) sp.decided(v, k, e);
            }
            first = false;
        }
        printf("%s %d %s\n", VERDICT[v], lc.n_iter(), FINAL[sp.final_step()]);
        delete[] errs;
    }
    return 0;
}
'''


@pytest.fixture(scope='module')
def program(tmp_path_factory):
    d = tmp_path_factory.mktemp('finish_in_pass')
    src, exe = d / 'final_step.cpp', d / 'final_step'
    src.write_text(PROGRAM)
    subprocess.check_call([os.environ.get('CXX', 'c++'), '-std=c++17', '-Wall', '-I', CSRC, str(src), '-o', str(exe)])
    return str(exe)


def expected(errs, thresh, max_n_iter, guess, fused, stores, finish):
    """step_03_apply_to_era.py:186-189, 308-319 on the scripted maxima, the launch plan as DESIGN.md states it, and the rule:
    NOTHING exactly when the chosen pass ends a launch that stored and finished and its maximum is a number."""
    it, n_iter, raised, last = 1, 0, False, math.inf
    for e in errs:
        if not last > thresh:
            break
        last = e
        n_iter += 1
        it += 1
        if it > max_n_iter:
            raised = True
            break
    if raised:
        return 'NOT_CONVERGED', n_iter, 'ALL_LEVELS'
    ends, done, first = {}, 0, True                                    # last pass of each launch -> did it store
    while done < n_iter:
        np_ = min(max(min(guess, MAX_PASS, max_n_iter), 1), max_n_iter - done) if first else min(2, max_n_iter - done)
        np_ = max(np_, 1)
        done += np_
        ends[done] = bool(stores) and not (first and fused and np_ == 1)
        first = False
    if not ends.get(n_iter, False):
        return 'CONVERGED', n_iter, 'ALL_LEVELS'
    if not finish:
        return 'CONVERGED', n_iter, 'ABOVE_MARKS'
    return 'CONVERGED', n_iter, 'ALL_LEVELS' if last != last else 'NOTHING'


def test_the_transcription_itself():
    up = [9.0, 8.0, 7.0, 6.0, 5.0]
    assert expected(up + [0.1] * 8, 1.0, 20, 6, 1, 1, 1) == ('CONVERGED', 6, 'NOTHING')
    assert expected(up + [0.1] * 8, 1.0, 20, 6, 1, 1, 0) == ('CONVERGED', 6, 'ABOVE_MARKS')
    assert expected(up + [0.1] * 8, 1.0, 20, 7, 1, 1, 1) == ('CONVERGED', 6, 'ALL_LEVELS')
    assert expected(up + [0.1] * 8, 1.0, 20, 4, 1, 1, 1) == ('CONVERGED', 6, 'NOTHING')
    assert expected(up + [0.1] * 8, 1.0, 20, 5, 1, 1, 1) == ('CONVERGED', 6, 'ALL_LEVELS')
    assert expected(up + [math.nan] * 8, 1.0, 20, 6, 1, 1, 1) == ('CONVERGED', 6, 'ALL_LEVELS')
    assert expected(up + [0.1] * 8, 1.0, 6, 6, 1, 1, 1) == ('NOT_CONVERGED', 6, 'ALL_LEVELS')
    assert expected([0.1] * 8, 1.0, 20, 1, 1, 1, 1) == ('CONVERGED', 1, 'ALL_LEVELS')     # the flagged kernel alone
    assert expected([0.1] * 8, 1.0, 20, 1, 0, 1, 1) == ('CONVERGED', 1, 'NOTHING')


def test_nothing_is_launched_exactly_when_the_rule_says_so(program):
    """Every file length 1 .. 11 against every first-launch size, with and without a fused first launch, a loop that stores
    or not (float32 fast mode, local p_ref), the option on and off; the chosen pass's maximum a number below the threshold,
    equal to it, or NaN; and max_n_iter at and next to the file's length."""
    cases = []
    for n in range(1, 12):
        for last in (0.5, 1.0, math.nan):
            errs = [9.0 - 0.01 * i for i in range(n - 1)] + [last] + [0.25] * 8
            for guess in (0, 1, 2, 3, 5, 6, 8, 9):
                for max_n_iter in (n, n + 1, 20):
                    for fused, stores, finish in ((1, 1, 1), (0, 1, 1), (1, 1, 0), (0, 0, 1), (1, 0, 0)):
                        cases.append((errs, 1.0, max_n_iter, guess, fused, stores, finish))
    lines = ['%r %d %d %d %d %d %d %s' % (c[1], c[2], c[3], c[4], c[5], c[6], len(c[0]), ' '.join(repr(e) for e in c[0]))
             for c in cases]
    out = subprocess.run([program], input=''.join(s + '\n' for s in lines).encode(), stdout=subprocess.PIPE, check=True)
    got = out.stdout.decode().splitlines()
    assert len(got) == len(cases)
    seen = set()
    for c, g in zip(cases, got):
        verdict, n_iter, final = g.split()
        assert (verdict, int(n_iter), final) == expected(*c), (c, g)
        seen.add(final)
    assert seen == {'NOTHING', 'ABOVE_MARKS', 'ALL_LEVELS'}
