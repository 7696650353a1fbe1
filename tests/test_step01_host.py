"""CPU-side checks of step_01 (pgw4era5_amd/step_01_extract_deltas.py): fixtures, level bookkeeping, command line.
No compute call is made here; the kernels are checked in tests/test_step01_hip.py."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden')


def _vectors():
    z = dict(np.load(os.path.join(GOLDEN, 'ref_step01_vectors.npz'), allow_pickle=False))
    with open(os.path.join(GOLDEN, 'ref_step01_vectors.json')) as f:
        return z, json.load(f)


def test_new_entries_are_declared_bound_and_have_kernel_ids():
    from pgw4era5_amd import _lib
    hdr = open(os.path.join(ROOT, 'include', 'pgw_hip.h')).read()
    for name in ('pgw_interp_hybrid_to_plev', 'pgw_magnus_rh', 'pgw_hur_merge_levels'):
        assert name in _lib.SIGNATURES and name + '(' in hdr
    for kid, cname in (('hybrid_to_plev', 'PGW_K_HYBRID_TO_PLEV'), ('magnus_rh', 'PGW_K_MAGNUS_RH'), ('hur_merge', 'PGW_K_HUR_MERGE')):
        assert '%s = %d' % (cname, _lib.KERNEL_IDS[kid]) in hdr
    assert 'PGW_K_COUNT = %d' % len(_lib.KERNEL_IDS) in hdr
    assert len(set(_lib.KERNEL_IDS.values())) == len(_lib.KERNEL_IDS)


def test_target_list_fixture():
    from pgw4era5_amd import step_01_extract_deltas as s1
    p = s1.load_target_plev(os.path.join(GOLDEN, 'CFday_target_p_MPI-ESM1-2-HR.dat'))
    assert p.dtype == np.float64 and p.shape == (99,)
    assert np.all(np.diff(p) > 0) and p[0] > 0 and p[-1] == 101000.0
    assert os.path.getsize(os.path.join(GOLDEN, 'CFday_target_p_MPI-ESM1-2-HR.dat')) < 1024


def test_golden_magnus_vectors_are_the_literal_numpy_expression():
    """Pins the fixture (outputs of the reference's own function) and the dtype flow the Magnus kernel implements:
    float32 QV / T with a float64 P give a float64 result in which the exponent, exp and the reciprocal are float32."""
    z, meta = _vectors()
    for tag, dt in (('f64', np.float64), ('f32', np.float32)):
        QV, P, T, RH = (z['%s_%s' % (tag, k)] for k in ('QV', 'P', 'T', 'RH'))
        assert QV.dtype == dt and T.dtype == dt and P.dtype == np.float64 and RH.dtype == np.float64
        assert meta['cases'][tag] == dict(QV=str(np.dtype(dt)), P='float64', T=str(np.dtype(dt)), RH='float64', n=len(RH))
        assert len(RH) >= 2000 and T.min() == dt(180.) and T.max() == dt(330.)
        lit = 0.263 * P * QV * (np.exp(17.67 * (T - 273.15) / (T - 29.65)))**(-1)
        assert lit.dtype == RH.dtype and np.array_equal(lit, RH)
        assert np.all(np.isfinite(RH)) and np.all(RH > 0)
    # the float32 case written out operation by operation
    QV, P, T, RH = (z['f32_%s' % k] for k in ('QV', 'P', 'T', 'RH'))
    a = np.float32(17.67) * (T - np.float32(273.15)) / (T - np.float32(29.65))
    r = np.float32(1) / np.exp(a)
    assert a.dtype == np.float32 and r.dtype == np.float32
    assert np.array_equal(0.263 * P * QV.astype(np.float64) * r.astype(np.float64), RH)
    # and it is not the float64 evaluation of the same inputs
    f64 = 0.263 * P * QV.astype(np.float64) * (np.exp(17.67 * (T.astype(np.float64) - 273.15) / (T.astype(np.float64) - 29.65)))**(-1)
    assert not np.array_equal(f64, RH)


def _emon_levels():
    """CMIP6 plev19 inside a finer Emon-like list: two extra levels in every plev19 interval down to 100 hPa."""
    from pgw4era5_amd.synthetic import PLEV19
    amon = np.asarray(PLEV19, dtype=np.float64)
    emon = [amon[0]]
    for lo, hi in zip(amon[:-1], amon[1:]):
        if lo > 10000.:
            emon += [lo + (hi - lo) / 3., lo + 2. * (hi - lo) / 3.]
        emon.append(hi)
    return np.array(emon), amon


def test_merge_level_table_on_plev19_inside_a_finer_list():
    from pgw4era5_amd import step_01_extract_deltas as s1
    emon, amon = _emon_levels()
    assert len(amon) == 19 and len(emon) > 40 and np.all(np.diff(emon) < 0)
    copy_from, e_above, e_below, a_above, a_below = s1.merge_level_table(emon, amon)
    for t in (copy_from, e_above, e_below, a_above, a_below):
        assert t.dtype == np.int32 and t.shape == emon.shape
    for l, p in enumerate(emon):
        if p in amon:
            assert amon[copy_from[l]] == p
            assert e_above[l] == e_below[l] == a_above[l] == a_below[l] == -1
        else:
            assert copy_from[l] == -1
            # nearest Amon level of higher (below) / lower (above) pressure, and the same pressures on the Emon axis
            assert amon[a_below[l]] == amon[amon > p].min() and amon[a_above[l]] == amon[amon < p].max()
            assert emon[e_below[l]] == amon[a_below[l]] and emon[e_above[l]] == amon[a_above[l]]
            assert a_above[l] == a_below[l] + 1                    # plev19 descends
    assert (copy_from >= 0).sum() == 19
    # order of the axes does not matter (ascending lists give the same pressures)
    t2 = s1.merge_level_table(emon[::-1], amon[::-1])
    assert np.array_equal(emon[::-1][t2[1][::-1][copy_from < 0]], emon[e_above[copy_from < 0]])


def test_merge_level_table_host_errors():
    from pgw4era5_amd import step_01_extract_deltas as s1
    emon, amon = _emon_levels()
    with pytest.raises(ValueError):                                # an Emon level below the lowest Amon level
        s1.merge_level_table(np.concatenate([[101000.], emon]), amon)
    with pytest.raises(ValueError):                                # ... above the highest
        s1.merge_level_table(np.concatenate([emon, [50.]]), amon)
    drop = np.nonzero(emon == 85000.)[0][0]                        # Amon level 850 hPa is no Emon level: its neighbours need it
    with pytest.raises(KeyError):
        s1.merge_level_table(np.delete(emon, drop), amon)


def test_argument_surface_of_both_sub_commands():
    from pgw4era5_amd import step_01_extract_deltas as s1
    p = s1.build_parser()
    a = p.parse_args(['interp_to_plev', '-i', 'in_{}.nc', '-o', 'out_{}.nc', '-v', 'ta,hur,ua,va', '-p', 'levels.dat'])
    assert (a.command, a.input, a.output, a.var_names, a.target_p) == ('interp_to_plev', 'in_{}.nc', 'out_{}.nc', 'ta,hur,ua,va', 'levels.dat')
    assert a.extrapolate == 'constant' and a.max_records is None and a.out_dtype is None
    a = p.parse_args(['interp_to_plev', '-i', 'a', '-o', 'b', '-v', 'ta', '-p', 'c', '--max_records', '3', '-x', 'nan'])
    assert a.max_records == 3 and a.extrapolate == 'nan'
    h = p.parse_args(['hus_to_hur', 'hus.nc', 'ta.nc', 'hur.nc', '-a', 'amon.nc'])
    assert (h.command, h.hus_file, h.ta_file, h.hur_file, h.amon_hur_file) == ('hus_to_hur', 'hus.nc', 'ta.nc', 'hur.nc', 'amon.nc')
    for bad in (['interp_to_plev', '-i', 'a'], ['hus_to_hur', 'hus.nc'], ['hus_to_hur', 'a', 'b', 'c'], []):
        with pytest.raises(SystemExit):
            p.parse_args(bad)
    with pytest.raises(ValueError):                                # several variables, no {} in the paths
        s1.main(['interp_to_plev', '-i', 'a.nc', '-o', 'b.nc', '-v', 'ta,ua', '-p', 'c'])


def test_help_runs_without_the_library():
    env = dict(os.environ, PGW_LIB=os.path.join(ROOT, 'no_such_dir', 'libpgw_hip.so'), PYTHONPATH=ROOT)
    for argv in (['--help'], ['interp_to_plev', '--help'], ['hus_to_hur', '--help']):
        r = subprocess.run([sys.executable, '-m', 'pgw4era5_amd.step_01_extract_deltas'] + argv, cwd=ROOT, env=env,
                           capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        assert 'usage' in r.stdout


def test_levels_descend_and_argument_checks_before_any_launch():
    from pgw4era5_amd import step_01_extract_deltas as s1
    ap = np.array([0., 2000., 8000., 5000., 100.])
    b = np.array([1., 0.9, 0.4, 0., 0.])
    assert s1.levels_descend(ap, b) and not s1.levels_descend(ap[::-1], b[::-1])
    var, ps = np.zeros((1, 5, 2, 3), np.float32), np.zeros((1, 2, 3), np.float32)
    with pytest.raises(ValueError):
        s1.interp_to_plev(var, ps, ap, b, [5e4], extrapolate='cubic')
    with pytest.raises(ValueError):
        s1.interp_to_plev(var, ps[:, :1], ap, b, [5e4])
    with pytest.raises(ValueError):
        s1.interp_to_plev(var, ps, ap[:4], b[:4], [5e4])
    with pytest.raises(ValueError):
        s1.interp_to_plev(var.astype(np.float64), ps, ap, b, [5e4], out_dtype='float32')
