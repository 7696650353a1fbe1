"""GPU tests of the surface riders (step_03:103-146, functions.py:1145-1186) at their masks, clips and mixed time axes:
`pgw_surface_update` (k_surface_update_lerp), `pgw_surface_deltas` (k_surface_deltas), the production kernel inside
`pgw_step03_file` (k_surface_update_lerp) and `F.integrate_tos` (k_integrate_tos, k_integrate_tos_mixed), all on the edge
inputs of tests/surface_edge_cases.py (checked on the CPU by tests/test_surface_riders_host.py).

Bounds.  The kernels and numpy perform the same IEEE operations in the same order and the library is built with
-ffp-contract=off, so everything that is arithmetic only is asserted bit for bit (assert_array_equal: NaN positions
included).  The soil weight exp(-z / 2.8) is the C library's exp on one side and numpy's on the other: rtol = atol = 1e-9,
the project's bound for float64 fields against these oracles (tests/test_hip_files.py, tests/test_step03_debug_hip.py);
in float32 storage one float32 ulp around the rounded oracle.  The float64 debug deltas of `pgw_surface_deltas` take the
same 1e-9 in every mode."""
import datetime as dt
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import surface_edge_cases as E                                                       # noqa: E402
from oracle import pgw_oracle as O                                                   # noqa: E402
from oracle import pgw_oracle_refdtype as R                                          # noqa: E402

pytestmark = pytest.mark.gpu

STORAGE = ('float64', 'float32')
LERP, RECORD = dt.datetime(2006, 8, 2, 3), dt.datetime(2006, 3, 15, 12)      # between two monthly records; ON the third
INSTANTS = dict(lerp=LERP, record=RECORD)
OUTPUTS = ('sic', 'comb', 'tskin', 'tso')
SENTINEL = -12345.0
F32_IDENTICAL = {}           # output -> [float32 results equal to the rounded oracle, float32 results]
MIXED_MAX = {}               # (mode, records hit) -> max relative difference of delta_ts_combined


@pytest.fixture(scope='module')
def gpu():
    from pgw4era5_amd import step_03_apply_to_era as s3, step_03_debug as dbg
    from pgw4era5_amd.device import default_context
    yield s3, dbg, default_context()
    if F32_IDENTICAL:
        print('\nfloat32 pgw_surface_update results bit-identical to the rounded oracle: ' +
              ', '.join('%s %d/%d (%.2f %%)' % (k, a, b, 100.0 * a / b) for k, (a, b) in sorted(F32_IDENTICAL.items())))
    for (mode, on), v in sorted(MIXED_MAX.items()):
        print('mixed axes %-13s records of {%s}: max rel diff of delta_ts_combined %.3e' % (mode, ', '.join(on), v))


def bits(x):
    return np.ascontiguousarray(x).view(np.uint64 if x.dtype == np.float64 else np.uint32)


def step0(inp):
    """The first time step of a build as a one-step build (same numbers)."""
    import types
    one = types.SimpleNamespace(**vars(inp))
    one.ntime = 1
    for k in ('sic', 'dsic', 'dtos', 'dts', 'tskin', 'tso', 'nan_ice', 'nan_comb', 'nan_soil'):
        setattr(one, k, getattr(inp, k)[:1].copy())
    return one


def surface_update(ctx, inp, outputs=OUTPUTS, nsoil=None, tskin=True, pad=0):
    """pgw_surface_update as step_03_apply_to_era.process_file_device_reinterp_composed calls it; outputs not named are
    passed as NULL.  `pad`: tso_out gets that many extra elements; all of it is pre-filled with SENTINEL and returned flat."""
    from pgw4era5_amd import _lib
    from pgw4era5_amd.device import dtype_tag
    T = inp.dtype
    nt, ncol = inp.sic.shape
    nsoil = inp.nsoil if nsoil is None else nsoil
    d = {k: ctx.to_device(np.ascontiguousarray(getattr(inp, k)), T) for k in ('sic', 'dsic', 'dtos', 'dts', 'land', 'clim', 'tskin', 'tso')}
    shapes = dict(sic=(nt, ncol), comb=(nt, ncol), tskin=(nt, ncol), tso=(nt * inp.nsoil * ncol + pad,) if pad else (nt, inp.nsoil, ncol))
    out = {k: ctx.empty(shapes[k], T) for k in outputs}
    for v in out.values():
        v.copy_from(np.full(v.shape, SENTINEL, dtype=T))
    soil = np.ascontiguousarray(inp.soil, dtype=np.float64)
    p = lambda k: out[k].ptr if k in out else None
    try:
        ctx._check(ctx.lib.pgw_surface_update(ctx.handle, dtype_tag(T), nt, ncol, nsoil, soil.ctypes.data_as(_lib._dp), d['sic'].ptr,
                                              d['dsic'].ptr, d['dtos'].ptr, d['dts'].ptr, d['land'].ptr, d['clim'].ptr,
                                              d['tskin'].ptr if tskin else None, d['tso'].ptr, p('sic'), p('comb'), p('tskin'), p('tso')))
        return {k: v.numpy() for k, v in out.items()}
    finally:
        for v in list(d.values()) + list(out.values()):
            v.free()


def within_one_f32_ulp(got, want32):
    lo, hi = np.nextafter(want32, np.float32(-np.inf)), np.nextafter(want32, np.float32(np.inf))
    nan = np.isnan(want32)
    np.testing.assert_array_equal(np.isnan(got), nan)
    assert np.all((got[~nan] >= lo[~nan]) & (got[~nan] <= hi[~nan]))


def check_update(got, want, dtype, what=''):
    """float64 storage: sic, comb, tskin equal to the oracle, tso at 1e-9.  float32 storage: the float64 oracle rounded once
    (the kernel computes in float64 on the stored values and rounds each output once), tso within one float32 ulp of it."""
    for k, g in got.items():
        assert g.dtype == np.dtype(dtype) and g.shape == want[k].shape, (k, g.dtype, g.shape)
        if dtype == 'float64':
            if k == 'tso':
                np.testing.assert_array_equal(np.isnan(g), np.isnan(want[k]), err_msg=what + k)
                np.testing.assert_allclose(g, want[k], rtol=1e-9, atol=1e-9, equal_nan=True, err_msg=what + k)
            else:
                np.testing.assert_array_equal(g, want[k], err_msg=what + k)
        else:
            w32 = want[k].astype(np.float32)
            if k == 'tso':
                within_one_f32_ulp(g, w32)
            else:
                np.testing.assert_array_equal(g, w32, err_msg=what + k)
            n = F32_IDENTICAL.setdefault(k, [0, 0])
            n[0] += int(np.sum((g == w32) | (np.isnan(g) & np.isnan(w32))))
            n[1] += g.size


# ================================================================== 2. pgw_surface_update against the oracle
@pytest.mark.parametrize('ntime', [1, 3])
@pytest.mark.parametrize('ncol', E.NCOLS)
@pytest.mark.parametrize('dtype', STORAGE)
def test_surface_update_vs_oracle(gpu, dtype, ncol, ntime):
    """k_surface_update_lerp on the edge table, 1 / 64 / 257 / 300 columns, one and three time steps, 1, 4 and 16 soil layers,
    against O.sea_ice_update, O.integrate_tos (land and the updated ice of time step 0 at every step, step_03:121-122),
    tskin + comb and tso + O.soil_temperature_delta in float64 on the float64-cast inputs."""
    s3, dbg, ctx = gpu
    for nsoil in E.NSOILS:
        inp = E.build(ncol, dtype, nsoil=nsoil, ntime=ntime)
        want = E.oracle_update(inp)
        got = surface_update(ctx, inp)
        check_update(got, want, dtype, 'nsoil %d ' % nsoil)
        np.testing.assert_array_equal(np.isnan(got['sic']), inp.nan_ice)
        np.testing.assert_array_equal(np.isnan(got['comb']), inp.nan_comb)
        np.testing.assert_array_equal(np.isnan(got['tso']), inp.nan_soil)
        if ncol >= len(E.NAMES):                 # the table's own words: clipped to 0 / 1 exactly, pure ts, pure tos
            for c, (name, ik, ck) in enumerate(zip(inp.names, inp.ice_kind, inp.comb_kind)):
                ice, comb = got['sic'][0, c], got['comb'][0, c]
                assert dict(nan=np.isnan(ice), zero=ice == 0, one=ice == 1, open=0 < ice < 1)[ik], (name, ice)
                assert dict(nan=np.isnan(comb), ts=comb == inp.dts[0, c], tos=comb == inp.dtos[0, c], finite=np.isfinite(comb))[ck], (name, comb)


@pytest.mark.parametrize('ncol', [257, 300])
@pytest.mark.parametrize('dtype', STORAGE)
def test_surface_update_time_steps(gpu, dtype, ncol):
    """Slab 0 of a three-step call is the one-step call bit for bit; slabs 1 and 2 blend with slab 0's ice (the oracle of
    test_surface_update_vs_oracle) while sic_out is their own - the slabs' sic and dsic differ, so a blend with the
    step's own ice, or with another step's, gives another result."""
    s3, dbg, ctx = gpu
    inp = E.build(ncol, dtype, nsoil=4, ntime=3)
    got3, got1 = surface_update(ctx, inp), surface_update(ctx, step0(inp))
    for k in OUTPUTS:
        np.testing.assert_array_equal(bits(got3[k][:1]), bits(got1[k]), err_msg=k)
    want = E.oracle_update(inp)
    check_update(got3, want, dtype)
    own = O.integrate_tos(E.f64(inp.dtos), E.f64(inp.dts), np.broadcast_to(E.f64(inp.land)[None], inp.dtos.shape), want['sic'])
    for t in (1, 2):
        assert not np.array_equal(want['sic'][t], want['sic'][0], equal_nan=True)
        differ = ~((own[t] == want['comb'][t]) | (np.isnan(own[t]) & np.isnan(want['comb'][t])))
        assert differ.sum() > ncol // 4, differ.sum()                 # the wrong slab would show in many columns
        one = step0(inp)
        one.sic, one.dsic = inp.sic[t:t + 1], inp.dsic[t:t + 1]
        np.testing.assert_array_equal(got3['sic'][t], E.oracle_update(one)['sic'][0].astype(dtype))   # sic_out: the step's own


@pytest.mark.parametrize('dtype', STORAGE)
def test_surface_update_optional_outputs(gpu, dtype):
    """Each of sic_out, dts_comb_out, tskin_out, tso_out may be NULL on its own: the others keep the bits of the full call."""
    s3, dbg, ctx = gpu
    inp = E.build(300, dtype, nsoil=4, ntime=3)
    full = surface_update(ctx, inp)
    for drop in OUTPUTS:
        got = surface_update(ctx, inp, outputs=[k for k in OUTPUTS if k != drop])
        assert sorted(got) == sorted(k for k in OUTPUTS if k != drop)
        for k, g in got.items():
            np.testing.assert_array_equal(bits(g), bits(full[k]), err_msg='%s without %s' % (k, drop))
    only = surface_update(ctx, inp, outputs=['comb'], tskin=False)           # no tskin_out: tskin itself may be NULL
    np.testing.assert_array_equal(bits(only['comb']), bits(full['comb']))


@pytest.mark.parametrize('dtype', STORAGE)
def test_surface_update_sixteen_soil_layers_and_the_end_of_tso(gpu, dtype):
    """nsoil = MAX_SOIL = 16, three time steps: every layer lands at (t * nsoil + s) * ncol + c (the unrolled loop's guard
    s < soil.n lets all 16 through), and the elements behind the end of tso_out keep their sentinel."""
    s3, dbg, ctx = gpu
    for ncol in (257, 300):
        inp = E.build(ncol, dtype, nsoil=16, ntime=3)
        want = E.oracle_update(inp)
        pad = ncol + 7
        flat = surface_update(ctx, inp, pad=pad)['tso']
        n = 3 * 16 * ncol
        assert flat.shape == (n + pad,)
        np.testing.assert_array_equal(flat[n:], np.full(pad, SENTINEL, dtype=dtype))
        tso = flat[:n].reshape(3, 16, ncol)
        assert not np.any(tso == np.dtype(dtype).type(SENTINEL))
        check_update(dict(tso=tso), want, dtype)
        deep = E.f64(inp.tso)[:, 15] + E.f64(inp.clim)[None]          # w = 0 at depth: tso + clim wherever comb is a number
        np.testing.assert_array_equal(tso[:, 15][~inp.nan_comb], deep.astype(dtype)[~inp.nan_comb])


@pytest.mark.parametrize('dtype', STORAGE)
def test_surface_update_statuses(gpu, dtype):
    """Bad arguments come back as the entry's ValueError, and the context computes the same bits afterwards."""
    from pgw4era5_amd import _lib
    s3, dbg, ctx = gpu
    inp = E.build(64, dtype, nsoil=4)
    before = surface_update(ctx, inp)
    for kw, msg in ((dict(nsoil=17), 'pgw_surface_update: nsoil must be in [0, 16]'),
                    (dict(tskin=False), 'pgw_surface_update: tskin required for tskin_out'),
                    (dict(nsoil=0), 'pgw_surface_update: tso, ts_clim, soil_depth required for tso_out')):
        with pytest.raises(ValueError) as e:
            surface_update(ctx, inp, **kw)
        assert str(e.value) == msg and e.value.status == _lib.PGW_ERR_ARG, kw
        after = surface_update(ctx, inp)
        for k in OUTPUTS:
            np.testing.assert_array_equal(bits(after[k]), bits(before[k]), err_msg=k)


# ================================================================== 3. pgw_surface_deltas on the edge inputs and on mixed axes
def device_surface_deltas(gpu, c, mode):
    """pgw_surface_deltas through step_03_debug.surface_deltas_device on the records and time axes of the case `c`.
    Returns (delta_ts_combined, delta_soilt, the annual-mean ts delta as the oracle of the mode takes it)."""
    s3, dbg, ctx = gpu
    dtype = np.dtype(E.DTYPE[mode])
    times = c['delta_times']
    ds = (s3.DeltaSet(ctx, c['deltas'], times.get('ta'), c['plev'], dtype, times_by_var=times) if isinstance(times, dict) else
          s3.DeltaSet(ctx, c['deltas'], times, c['plev'], dtype))
    era = {k: ctx.to_device(np.ascontiguousarray(c['era'][k], dtype=dtype), dtype) for k in ('FR_SEA_ICE', 'FR_LAND')}
    try:
        clim = ds.ts_clim.numpy()
        ts, st = dbg.surface_deltas_device(ctx, era, dict(soil1=c['era']['soil1']), ds, c['target_dt'], mode == 'f32_reference')
        return ts.numpy(), st.numpy(), clim if mode == 'f32_reference' else clim.astype(np.float64)
    finally:
        ds.free()
        for v in era.values():
            v.free()


def check_deltas(got_ts, got_st, want_ts, want_st, what):
    assert got_ts.dtype == np.float64 and got_st.dtype == np.float64
    assert got_ts.shape == want_ts.shape and got_st.shape == want_st.shape, what
    np.testing.assert_array_equal(np.isnan(got_ts), np.isnan(want_ts), err_msg='NaN mask of delta_ts_combined ' + what)
    np.testing.assert_array_equal(np.isnan(got_st), np.isnan(want_st), err_msg='NaN mask of delta_soilt ' + what)
    np.testing.assert_allclose(got_ts, want_ts, rtol=1e-9, atol=1e-9, equal_nan=True, err_msg='delta_ts_combined ' + what)
    np.testing.assert_allclose(got_st, want_st, rtol=1e-9, atol=1e-9, equal_nan=True, err_msg='delta_soilt ' + what)


def max_rel(got, want):
    ok = np.isfinite(want) & (want != 0)
    return float(np.max(np.abs(got[ok] - want[ok]) / np.abs(want[ok]))) if ok.any() else 0.0


@pytest.mark.parametrize('instant', list(INSTANTS))
@pytest.mark.parametrize('mode', E.MODES)
def test_surface_deltas_on_the_edge_inputs(gpu, mode, instant):
    """The edge inputs as the records of a DeltaSet, an instant between two records and one on a record: delta_ts_combined
    and delta_soilt against oracle_surface_deltas; NaN exactly where the construction predicts (a NaN ts record makes the
    annual mean NaN too, in columns whose blend is NaN already)."""
    for ncol, nsoil in [(n, 4) for n in E.NCOLS] + [(300, 1), (300, 16)]:
        inp = E.build(ncol, E.DTYPE[mode], nsoil=nsoil)
        c = E.delta_case(inp, INSTANTS[instant])
        ts, st, clim = device_surface_deltas(gpu, c, mode)
        want_ts, want_st = E.oracle_surface_deltas(c, mode, clim)
        check_deltas(ts, st, want_ts, want_st, '%s %s ncol %d nsoil %d' % (mode, instant, ncol, nsoil))
        np.testing.assert_array_equal(np.isnan(ts).reshape(1, ncol), inp.nan_comb)
        np.testing.assert_array_equal(np.isnan(st).reshape(1, nsoil, ncol), inp.nan_soil)
        assert ncol < len(E.NAMES) or (np.isnan(ts).any() and not np.isnan(ts).all())
        if ncol >= len(E.NAMES):       # the table survives the time interpolation: pure ts / pure tos columns are those records
            for k, (name, ck) in enumerate(zip(inp.names, inp.comb_kind)):
                if ck in ('ts', 'tos'):
                    assert ts[0, 0, k] == (inp.dts if ck == 'ts' else inp.dtos)[0, k], (name, ts[0, 0, k])


@pytest.mark.parametrize('instant', list(INSTANTS))
@pytest.mark.parametrize('mode', E.MODES)
def test_surface_deltas_three_time_steps(gpu, mode, instant):
    """pgw_surface_deltas called directly with ntime = 3 (records of three slabs): every step blends with the updated ice of
    time step 0; the slabs' sic and siconc differ, so the wrong slab shows."""
    from pgw4era5_amd import _lib
    from pgw4era5_amd.device import dtype_tag
    s3, dbg, ctx = gpu
    T = np.dtype(E.DTYPE[mode])
    ora = R if mode == 'f32_reference' else O
    times = E.DELTA_TIMES[6:8]                                    # 15 July and 15 August
    target = LERP if instant == 'lerp' else dt.datetime(2006, 7, 15, 12)
    ib, ia, x_hi, x_new, keep = s3.delta_time_bracket(times, target)
    assert (x_hi == 0.0) == (instant == 'record')
    for ncol in (257, 300):
        inp = E.build(ncol, T, nsoil=4, ntime=3)
        rec = E.records(inp, nrec=2)                              # (2, 3, ncol) each
        ld = lambda k: ora.load_delta_values((rec[k] if ora is R else E.f64(rec[k])).reshape(2, 3, 1, ncol), times, target)[0]
        clim = inp.clim if ora is R else E.f64(inp.clim)
        _, want_ts, want_st = E.surface_deltas_of(mode, inp.sic.reshape(3, 1, ncol), inp.land.reshape(1, 1, ncol), ld('siconc'), ld('tos'),
                                                  ld('ts'), clim.reshape(1, ncol), inp.soil)
        dev = {k: ctx.to_device(np.ascontiguousarray(v), T) for k, v in rec.items()}
        fix = {k: ctx.to_device(np.ascontiguousarray(getattr(inp, k)), T) for k in ('sic', 'land', 'clim')}
        ts, st = ctx.empty((3, 1, ncol), np.float64), ctx.empty((3, 4, 1, ncol), np.float64)
        args = []
        for k in ('siconc', 'tos', 'ts'):
            args += [dev[k].slab(int(keep[ib])).ptr, dev[k].slab(int(keep[ia])).ptr, x_hi, x_new]
        try:
            ctx._check(ctx.lib.pgw_surface_deltas(ctx.handle, dtype_tag(T), 1 if ora is R else 0, 3, ncol, 4, inp.soil.ctypes.data_as(_lib._dp),
                                                  fix['sic'].ptr, *args, fix['land'].ptr, fix['clim'].ptr, ts.ptr, st.ptr))
            got_ts, got_st = ts.numpy(), st.numpy()
        finally:
            for v in list(dev.values()) + list(fix.values()) + [ts, st]:
                v.free()
        check_deltas(got_ts, got_st, want_ts, want_st, '%s %s ncol %d' % (mode, instant, ncol))
        np.testing.assert_array_equal(np.isnan(got_ts).reshape(3, ncol), inp.nan_comb)


COMBOS = [tuple(v for i, v in enumerate(('siconc', 'tos', 'ts')) if (m >> i) & 1) for m in range(8)]


@pytest.mark.parametrize('on_record', COMBOS, ids=lambda on: '+'.join(on) or 'none')
@pytest.mark.parametrize('mode', ['f64', 'f32_reference'])
def test_surface_deltas_mixed_time_axes(gpu, mode, on_record):
    """All 8 combinations of {siconc, tos, ts} x {the instant is a record, the instant is interpolated}: every delta file has
    its own time axis (load_delta per variable), so in reference-dtype mode each of the three deltas is float32 (a record)
    or float64 (interpolated) on its own, and numpy promotes the ice update by siconc, each product of the blend by its
    delta and the sum by both (R.integrate_tos).  Against R / O fed load_delta_values of each variable on its own axis."""
    inp = E.build(300, E.DTYPE[mode], nsoil=4)
    c = E.mixed_axis_case(inp, on_record, LERP)
    ts, st, clim = device_surface_deltas(gpu, c, mode)
    want_ts, want_st = E.oracle_surface_deltas(c, mode, clim)
    MIXED_MAX[(mode, on_record)] = max_rel(ts, want_ts)
    print('%s records of {%s}: max rel diff dts %.3e dsoil %.3e' % (mode, ', '.join(on_record), max_rel(ts, want_ts), max_rel(st, want_st)))
    check_deltas(ts, st, want_ts, want_st, '%s records of %s' % (mode, on_record))


# ================================================================== 4. production tied to the debug kernel
@pytest.mark.parametrize('nsoil', [1, 16])
@pytest.mark.parametrize('dtype', STORAGE)
def test_surface_update_is_the_debug_deltas_bit_for_bit(gpu, dtype, nsoil):
    """pgw_surface_update and pgw_surface_deltas on the same exact records (x_hi = 0, no record after the instant), float64
    and float32 non-reference storage, three time steps, 257 and 300 columns, 1 and 16 soil layers: dts_comb_out is the
    float64 delta_ts_combined rounded to the storage type, tskin_out and tso_out are float64(era) + the float64 delta
    rounded once - the soil weights come from the same host exp on both sides, so tso is held bit for bit too."""
    from pgw4era5_amd import _lib
    from pgw4era5_amd.device import dtype_tag
    s3, dbg, ctx = gpu
    T = np.dtype(dtype)
    for ncol in (257, 300):
        inp = E.build(ncol, dtype, nsoil=nsoil, ntime=3)
        got = surface_update(ctx, inp)
        d = {k: ctx.to_device(np.ascontiguousarray(getattr(inp, k)), T) for k in ('sic', 'dsic', 'dtos', 'dts', 'land', 'clim')}
        ts, st = ctx.empty((3, ncol), np.float64), ctx.empty((3, nsoil, ncol), np.float64)
        soil = np.ascontiguousarray(inp.soil, dtype=np.float64)
        args = []
        for k in ('dsic', 'dtos', 'dts'):
            args += [d[k].ptr, None, 0.0, 0.0]
        try:
            ctx._check(ctx.lib.pgw_surface_deltas(ctx.handle, dtype_tag(T), 0, 3, ncol, nsoil, soil.ctypes.data_as(_lib._dp), d['sic'].ptr, *args, d['land'].ptr, d['clim'].ptr, ts.ptr, st.ptr))
            dts_comb, delta_soilt = ts.numpy(), st.numpy()
        finally:
            for v in list(d.values()) + [ts, st]:
                v.free()
        what = 'ncol %d ' % ncol
        np.testing.assert_array_equal(got['comb'], dts_comb.astype(T), err_msg=what + 'comb')
        np.testing.assert_array_equal(got['tskin'], (E.f64(inp.tskin) + dts_comb).astype(T), err_msg=what + 'tskin')
        np.testing.assert_array_equal(got['tso'], (E.f64(inp.tso) + delta_soilt).astype(T), err_msg=what + 'tso')
        np.testing.assert_array_equal(np.isnan(dts_comb), inp.nan_comb)
        np.testing.assert_array_equal(np.isnan(delta_soilt), inp.nan_soil)


AXES = dict(shared=(None, LERP), shared_record=(None, RECORD), siconc_on_record=(('siconc',), LERP), ts_on_record=(('ts',), LERP))


def file_case(dtype, on_record):
    """A tiny file of 6 x 50 = 300 columns and 12 levels whose surface fields and surface delta records are the edge inputs."""
    from pgw4era5_amd import synthetic
    c = synthetic.make_case(nlat=6, nlon=50, nlev=12, seed=17, dtype=np.dtype(dtype).type, nsoil=4)
    inp = E.build(300, dtype, nsoil=4)
    era = dict(c['era'])
    era.update(FR_SEA_ICE=inp.sic.reshape(1, 6, 50), FR_LAND=inp.land.reshape(1, 6, 50), T_SKIN=inp.tskin.reshape(1, 6, 50),
               T_SO=inp.tso.reshape(1, 4, 6, 50), soil1=inp.soil)
    deltas, times = dict(c['deltas']), c['delta_times']
    if on_record is not None:
        m = E.mixed_axis_case(inp, on_record, LERP)
        times = {k: c['delta_times'] for k in deltas}
        times.update({k: m['delta_times'][k] for k in ('siconc', 'tos', 'ts')})
    deltas.update({k: v.reshape(12, 6, 50) for k, v in E.records(inp).items()})
    return inp, dict(era=era, deltas=deltas, delta_times=times, plev=c['plev'])


@pytest.mark.parametrize('axes', list(AXES))
@pytest.mark.parametrize('mode', E.MODES)
def test_production_riders_are_the_debug_deltas_bit_for_bit(gpu, mode, axes):
    """pgw_step03_file (k_surface_update_lerp) on the edge inputs: FR_SEA_ICE is the oracle's update (exact in float64; in the
    float32 modes the value in the file dtype as the mode defines it: the float64 update rounded once in fast mode, the
    in-place float32 update in reference mode); T_SKIN and T_SO are float64(era) + the delta pgw_surface_deltas writes
    for the same records, cast to the file dtype, bit for bit - the two kernels share their expressions."""
    s3, dbg, ctx = gpu
    T = np.dtype(E.DTYPE[mode])
    on_record, target = AXES[axes]
    inp, c = file_case(T, on_record)
    c['target_dt'] = target
    ref = dict(f64=None, f32_fast=False, f32_reference=True)[mode]
    prod = s3.pgw_for_era5_arrays(c['era'], c['deltas'], c['delta_times'], c['plev'], target, True, ref_dtype=ref)
    dts, dst, clim = device_surface_deltas(gpu, c, mode)
    ora = R if mode == 'f32_reference' else O
    times = c['delta_times']
    ld = lambda k: ora.load_delta_values(c['deltas'][k] if ora is R else E.f64(c['deltas'][k]),
                                         times[k] if isinstance(times, dict) else times, target)
    sic, want_ts, want_st = E.surface_deltas_of(mode, c['era']['FR_SEA_ICE'], c['era']['FR_LAND'], ld('siconc'), ld('tos'), ld('ts'),
                                                clim, c['era']['soil1'])
    check_deltas(dts, dst, want_ts, want_st, '%s %s' % (mode, axes))
    assert prod['FR_SEA_ICE'].dtype == prod['T_SKIN'].dtype == prod['T_SO'].dtype == T
    np.testing.assert_array_equal(prod['FR_SEA_ICE'], sic.astype(T), err_msg='FR_SEA_ICE')
    np.testing.assert_array_equal(np.isnan(prod['FR_SEA_ICE']).reshape(1, 300), inp.nan_ice)
    np.testing.assert_array_equal(prod['T_SKIN'], (E.f64(c['era']['T_SKIN']) + dts).astype(T), err_msg='T_SKIN')
    np.testing.assert_array_equal(prod['T_SO'], (E.f64(c['era']['T_SO']) + dst).astype(T), err_msg='T_SO')
    np.testing.assert_array_equal(np.isnan(prod['T_SKIN']).reshape(1, 300), inp.nan_comb)
    if mode == 'f64':
        # settings.i_reinterp = 1: the one-call path runs the same kernel; the host-composed path interpolates the three
        # deltas first (DeltaSet.lerp2d: k_time_lerp, or a copy of the record) and calls pgw_surface_update on them - the
        # same float64 expressions in the same order, so the same bits
        again = s3.pgw_for_era5_arrays(c['era'], c['deltas'], c['delta_times'], c['plev'], target, True, i_reinterp=True)
        ds = (s3.DeltaSet(ctx, c['deltas'], times.get('ta'), c['plev'], T, times_by_var=times) if isinstance(times, dict) else
              s3.DeltaSet(ctx, c['deltas'], times, c['plev'], T))
        try:
            e = s3._upload_era(ctx, c['era'], T)
            coeffs = dict(ak=c['era']['ak'], bk=c['era']['bk'], soil1=c['era']['soil1'])
            comp, _ = s3.process_file_device_reinterp_composed(ctx, e, coeffs, ds, target, True)
            comp = {k: comp[k].numpy() for k in ('FR_SEA_ICE', 'T_SKIN', 'T_SO')}
        finally:
            ds.free()
        for k in ('FR_SEA_ICE', 'T_SKIN', 'T_SO'):
            np.testing.assert_array_equal(again[k], prod[k], err_msg='i_reinterp ' + k)
            np.testing.assert_array_equal(comp[k], prod[k], err_msg='i_reinterp, composed on the host: ' + k)


# ================================================================== 5. F.integrate_tos on the same table
@pytest.mark.parametrize('flow', ['common', 'reference'])
def test_integrate_tos_on_the_edge_table(gpu, flow, monkeypatch):
    """The flat k_integrate_tos (common flow: every operand cast to one dtype, float64 arithmetic, one rounding) against
    O.integrate_tos, and k_integrate_tos_mixed (reference flow: every operand in its own dtype) against R.integrate_tos, for
    the 16 operand dtype combinations tests/test_function_dtype_flow.py runs this entry with: exact, NaN masks included."""
    from pgw4era5_amd import functions as F, settings
    monkeypatch.setattr(settings, 'function_dtype_flow', flow)
    f4, f8 = np.float32, np.float64
    for ntime in (1, 3):
        inp = E.build(300, 'float64', ntime=ntime)
        ice = np.broadcast_to(O.sea_ice_update(inp.sic, inp.dsic)[0][None], inp.dtos.shape)
        ops = (inp.dtos, inp.dts, np.broadcast_to(inp.land[None], inp.dtos.shape), ice)
        for m in range(16):
            arrs = [np.ascontiguousarray(x.astype(f4 if (m >> i) & 1 else f8)) for i, x in enumerate(ops)]
            got = F.integrate_tos(*arrs)
            if flow == 'common':
                want = O.integrate_tos(*arrs).astype(f4 if m == 15 else f8)
            else:
                want = R.integrate_tos(*arrs)
            assert got.dtype == want.dtype and got.shape == want.shape, m
            np.testing.assert_array_equal(np.isnan(got), inp.nan_comb, err_msg='NaN mask, dtypes %d' % m)
            np.testing.assert_array_equal(got, want, err_msg='dtypes %d' % m)
