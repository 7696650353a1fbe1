"""Edge inputs of the surface riders (sea-ice update, tos / ts blend, skin and soil temperature; step_03:103-146,
functions.py:1145-1186) and their plain references, shared by tests/test_surface_riders_host.py (CPU) and
tests/test_surface_riders_hip.py (GPU).  A plain module: no fixtures, no pytest hooks.

`build(ncol, dtype, nsoil, ntime)` returns flat inputs whose first columns are the named table `edge_table(dtype)` - the
mask disagreements, the clips of the ice update and of the blend fraction at, beside and far from their bounds, the
float32 cancellation pair - and whose other columns are random but plausible (land columns with NaN sea ice and NaN tos,
open ocean, coast).  Every table value is a float32 number, so the float32 and the float64 build hold the same numbers
(except `one storage ulp beside 0 / 1`, which is an ulp of the requested dtype)."""
import types

import numpy as np

from oracle import pgw_oracle as O
from oracle import pgw_oracle_refdtype as R

NCOLS = (1, 64, 257, 300)        # one thread; a full wave; a one-thread and a ragged second block of 256 threads
NSOILS = (1, 4, 16)
ERA_DEPTHS = (0.035, 0.175, 0.64, 1.945)
MODES = ('f64', 'f32_fast', 'f32_reference')
DTYPE = dict(f64=np.float64, f32_fast=np.float32, f32_reference=np.float32)
DELTA_TIMES = np.array(['1995-%02d-15T12:00:00' % (m + 1) for m in range(12)], dtype='datetime64[s]')
PLEV = np.array([100000., 30000.])          # a DeltaSet wants a pressure axis; the surface deltas have none


def soil_depths(nsoil):
    """1: the surface itself (w = exp(0) = 1); 4: the ERA depths; 16 (the kernels' MAX_SOIL): depth 0, the ERA depths, ten
    deeper ones and one at which exp(-z / 2.8) underflows to 0."""
    if nsoil == 1:
        return np.array([0.0])
    if nsoil == 4:
        return np.array(ERA_DEPTHS)
    if nsoil == 16:
        z = np.array((0.0,) + ERA_DEPTHS + (2.89, 4.0, 6.0, 9.0, 13.5, 20.0, 30.0, 45.0, 70.0, 100.0, 1.0e4))
        assert len(z) == 16 and np.exp(-z[-1] / 2.8) == 0.0
        return z
    raise ValueError(nsoil)


def edge_table(dtype):
    """[(name, sic, dsic, tos is finite, ts is finite, land, ice, comb)]: `ice` is what the update gives ('nan', 'zero',
    'one', 'open' = strictly inside (0, 1)), `comb` what the blend gives ('nan', 'ts', 'tos' = that delta exactly,
    'finite')."""
    T = np.dtype(dtype).type
    f32 = np.float32
    nan, F, N = np.nan, True, False
    sub = float(np.nextafter(T(0), T(1)))                       # one storage ulp above 0: the smallest subnormal
    below1, above1 = float(np.nextafter(T(1), T(0))), float(np.nextafter(T(1), T(2)))
    c_sic = float(f32(0.2))
    c_lo, c_hi = float(np.nextafter(f32(-20), f32(-np.inf))), float(np.nextafter(f32(-20), f32(0)))
    return [
        # ---- the two halves of the mask ~isnan(ice) & ~isnan(tos), and NaN land / ts on either side of it
        ('sic_nan_tos_finite', nan, -5.0, F, F, 0.25, 'nan', 'ts'),
        ('sic_finite_tos_nan', 0.5, -5.0, N, F, 0.25, 'open', 'ts'),
        ('dsic_nan_sic_finite', 0.5, nan, F, F, 0.25, 'nan', 'ts'),
        ('both_nan', nan, -5.0, N, F, 1.0, 'nan', 'ts'),
        ('land_nan_in_mask', 0.5, -5.0, F, F, nan, 'open', 'nan'),         # np.clip keeps the NaN
        ('land_nan_out_mask', nan, -5.0, N, F, nan, 'nan', 'ts'),
        ('ts_nan_in_mask', 0.5, -5.0, F, N, 0.25, 'open', 'nan'),
        ('ts_nan_out_mask', nan, -5.0, F, N, 0.25, 'nan', 'nan'),
        # ---- clip of the ice update, sic + dsic / 100
        ('ice_exact_0', 0.25, -25.0, F, F, 0.5, 'zero', 'finite'),
        ('ice_exact_1', 0.75, 25.0, F, F, 0.0, 'one', 'ts'),
        ('ice_ulp_above_0', sub, 0.0, F, F, 0.0, 'open', 'tos'),          # frac > 0, yet 1 - frac rounds to 1
        ('ice_ulp_below_0', -sub, 0.0, F, F, 0.0, 'zero', 'tos'),
        ('ice_ulp_below_1', below1, 0.0, F, F, 0.0, 'open', 'finite'),
        ('ice_ulp_above_1', above1, 0.0, F, F, 0.0, 'one', 'ts'),
        ('ice_far_below_0', 0.125, -80.0, F, F, 0.5, 'zero', 'finite'),
        ('ice_far_above_1', 0.875, 80.0, F, F, 0.0, 'one', 'ts'),
        ('dsic_neg_zero', 0.5, -0.0, F, F, 0.25, 'open', 'finite'),
        # ---- clip of the blend fraction, ice + land
        ('frac_exact_1', 0.5, -25.0, F, F, 0.75, 'open', 'ts'),
        ('frac_exact_0', 0.25, -25.0, F, F, 0.0, 'zero', 'tos'),
        ('frac_above_1', 0.5, 0.0, F, F, 1.0, 'open', 'ts'),              # land = 1 and ice > 0
        ('pure_tos', 0.0, 0.0, F, F, 0.0, 'zero', 'tos'),                 # land = 0 and ice = 0
        ('pure_ts', 0.0, 0.0, F, F, 1.0, 'zero', 'ts'),                   # land = 1
        # ---- float32 cancellation: 0.2f + dsic / 100 one float32 ulp either side of -20
        ('cancel_below', c_sic, c_lo, F, F, 0.25, 'zero', 'finite'),
        ('cancel_above', c_sic, c_hi, F, F, 0.25, 'open', 'finite'),
    ]


NAMES = [row[0] for row in edge_table(np.float32)]


def build(ncol, dtype, nsoil=4, ntime=1, seed=5):
    """Flat surface inputs in `dtype`: sic, dsic, dtos, dts, tskin (ntime, ncol); land, clim (ncol); tso (ntime, nsoil, ncol);
    soil (nsoil,) float64 depths.  Columns [0, min(ncol, len(table))) of time step 0 are the table, the others random.
    Time steps 1, 2, ... hold step 0's sic, dsic, dtos and dts rolled along the columns by different strides (and the two
    temperature deltas shifted), so every step has every edge somewhere and no step repeats another.
    `nan_ice`, `nan_comb` (ntime, ncol) and `nan_soil` (ntime, nsoil, ncol) predict the NaNs of the three results from the
    construction alone; `ice_kind` / `comb_kind` are the table's expectations for time step 0."""
    dt = np.dtype(dtype)
    table = edge_table(dt)[:ncol]
    nt = len(table)
    rng = np.random.default_rng(seed + 1000 * ncol)
    # random columns: 30 % land (no sea ice, no tos), 20 % open ocean, the rest coast
    kind = rng.uniform(size=ncol)
    is_land, is_ocean = kind < 0.3, (kind >= 0.3) & (kind < 0.5)
    land = np.where(is_land, 1.0, np.where(is_ocean, 0.0, rng.uniform(0.02, 0.98, ncol)))
    sic = np.where(is_land, np.nan, rng.uniform(0.0, 1.0, ncol))
    dsic = rng.uniform(-30.0, 10.0, ncol)
    dtos = np.where(is_land, np.nan, 1.5 + 0.5 * rng.standard_normal(ncol))
    dts = 2.5 + 0.5 * rng.standard_normal(ncol)
    for c, (_, s, d, tos_ok, ts_ok, l, _, _) in enumerate(table):
        sic[c], dsic[c], land[c] = s, d, l
        dtos[c] = 1.0 + c / 16.0 if tos_ok else np.nan           # exact in float32, different in every column
        dts[c] = 2.0 + c / 8.0 if ts_ok else np.nan

    def steps(x, stride, shift=0.0):
        return np.stack([np.roll(x, stride * t) + shift * t if shift else np.roll(x, stride * t) for t in range(ntime)])   # keeps -0.0

    inp = types.SimpleNamespace(
        ncol=ncol, ntime=ntime, nsoil=nsoil, dtype=dt, names=[r[0] for r in table], ntable=nt,
        ice_kind=[r[6] for r in table], comb_kind=[r[7] for r in table],
        sic=steps(sic, 3).astype(dt), dsic=steps(dsic, 5).astype(dt), dtos=steps(dtos, 2, 0.25).astype(dt),
        dts=steps(dts, 7, 0.5).astype(dt), land=land.astype(dt), clim=(2.0 + 0.3 * rng.standard_normal(ncol)).astype(dt),
        tskin=(285.0 + 5.0 * rng.standard_normal((ntime, ncol))).astype(dt),
        tso=(283.0 + 5.0 * rng.standard_normal((ntime, nsoil, ncol))).astype(dt),
        soil=soil_depths(nsoil))
    inp.nan_ice = np.isnan(inp.sic) | np.isnan(inp.dsic)
    in_mask = ~inp.nan_ice[0][None] & ~np.isnan(inp.dtos)                         # ice of time step 0, step_03:121-122
    inp.nan_comb = np.where(in_mask, np.isnan(inp.land)[None] | np.isnan(inp.dts), np.isnan(inp.dts))
    inp.nan_soil = np.repeat(inp.nan_comb[:, None], nsoil, axis=1)
    return inp


def col(inp, name):
    return inp.names.index(name)


def f64(x):
    return np.asarray(x, dtype=np.float64)


# ------------------------------------------------------------------------------------------------------------------------
# plain references
# ------------------------------------------------------------------------------------------------------------------------
def oracle_update(inp):
    """What pgw_surface_update computes, by the float64 oracle on the float64-cast inputs: the sea-ice update, the blend
    with land and the UPDATED ice of time step 0 at every step (step_03:121-122), tskin + comb, tso + the soil delta."""
    nt, ncol = inp.sic.shape
    sic = O.sea_ice_update(f64(inp.sic), f64(inp.dsic))
    land0 = np.broadcast_to(f64(inp.land)[None], (nt, ncol))
    ice0 = np.broadcast_to(sic[0][None], (nt, ncol))
    comb = O.integrate_tos(f64(inp.dtos), f64(inp.dts), land0, ice0)
    dsoil = O.soil_temperature_delta(comb[:, None, :], f64(inp.clim)[None, :], inp.soil)[:, :, 0, :]
    return dict(sic=sic, comb=comb, tskin=f64(inp.tskin) + comb, tso=f64(inp.tso) + dsoil, dsoil=dsoil)


def surface_deltas_of(mode, sic, land, d_sic, d_tos, d_ts, clim, soil1):
    """delta_ts_combined (step_03:103-125) and delta_soilt (:139-143) from the deltas AT the instant (what load_delta_values
    of the mode's oracle returns, leading time axis included) by the oracle lines of the mode: 'f32_reference' takes
    the in-place float32 sea-ice update and R.integrate_tos on the arrays as they are, the other modes the float64 oracle
    on the widened values.  Land and the updated ice of time step 0 serve every time step.  Returns (sic, comb, dsoil)."""
    if mode == 'f32_reference':
        sic = np.array(sic, copy=True)
        with np.errstate(invalid='ignore'):
            np.add(sic, d_sic / 100, out=sic, casting='same_kind')                 # step_03:105
        sic = np.clip(sic, 0, 1)
        land0, tos, ts = np.asarray(land)[0], d_tos, d_ts
        blend = R.integrate_tos
    else:
        sic = O.sea_ice_update(f64(sic), f64(d_sic))
        land0, tos, ts = f64(land)[0], f64(d_tos), f64(d_ts)
        blend = O.integrate_tos
    shape = np.broadcast_shapes(tos.shape, (sic.shape[0],) + land0.shape)
    tos, ts = np.broadcast_to(tos, shape), np.broadcast_to(ts, shape)
    comb = blend(tos, ts, np.broadcast_to(land0, shape), np.broadcast_to(sic[0], shape))
    return sic, comb, O.soil_temperature_delta(comb, clim, soil1)


def oracle_surface_deltas(c, mode, clim):
    """step_03:103-125, 139-143 of a case dict (era, deltas, delta_times, target_dt) by the oracle lines of the mode; `clim`
    is the annual-mean ts delta handed to both sides.  `delta_times` may be a dict with one time axis per delta file
    (load_delta per variable, functions.py:195-303)."""
    ora = R if mode == 'f32_reference' else O
    times = c['delta_times']
    ld = lambda k: ora.load_delta_values(c['deltas'][k] if ora is R else f64(c['deltas'][k]),
                                         times[k] if isinstance(times, dict) else times, c['target_dt'])
    era = c['era']
    _, comb, dsoil = surface_deltas_of(mode, era['FR_SEA_ICE'], era['FR_LAND'], ld('siconc'), ld('tos'), ld('ts'), clim, era['soil1'])
    return comb, dsoil


# ------------------------------------------------------------------------------------------------------------------------
# the edge inputs as delta records
# ------------------------------------------------------------------------------------------------------------------------
def records(inp, nrec=12, seed=3):
    """siconc / tos / ts as `nrec` records each of shape (ntime, ncol) in the inputs' dtype: the table columns are the same in
    every record - an interpolation between two of them returns the value itself, (a - a) / x_hi * x_new + a, so the ties
    stay exact - and the random columns differ from record to record, so a wrong bracket shows.  NaNs stay NaN."""
    rng = np.random.default_rng(seed)
    out = {}
    for name, base, amp in (('siconc', inp.dsic, 2.0), ('tos', inp.dtos, 0.1), ('ts', inp.dts, 0.1)):
        noise = amp * rng.standard_normal((nrec,) + base.shape)
        noise[:, 0, :inp.ntable] = 0.0
        out[name] = (f64(base)[None] + noise).astype(inp.dtype)
    return out


def delta_case(inp, target_dt, nrec=12, delta_times=None):
    """The inputs as a file-shaped case for DeltaSet / oracle_surface_deltas: one time step, a grid of 1 x ncol."""
    assert inp.ntime == 1
    rec = records(inp, nrec)
    deltas = {k: v.reshape(nrec, 1, inp.ncol) for k, v in rec.items()}
    era = dict(FR_SEA_ICE=inp.sic.reshape(1, 1, inp.ncol), FR_LAND=inp.land.reshape(1, 1, inp.ncol), soil1=inp.soil)
    return dict(era=era, deltas=deltas, delta_times=DELTA_TIMES if delta_times is None else delta_times, plev=PLEV,
                target_dt=target_dt)


def mixed_axis_case(inp, on_record, target_dt):
    """delta_case with one time axis per variable (synthetic.resample_deltas): the variables in `on_record` get twelve
    stamps 30 days apart of which one IS the instant (re-yeared), the others keep the monthly axis, on which the instant
    lies between two records."""
    from pgw4era5_amd import synthetic
    c = delta_case(inp, target_dt)
    hit = np.datetime64(target_dt).astype('datetime64[s]')
    hit = np.datetime64('1995' + str(hit)[4:])
    stamps = {v: hit + (np.arange(12) - 7) * np.timedelta64(30, 'D') for v in on_record}
    _, times = synthetic.resample_deltas(c, stamps)
    for v in on_record:
        assert str(times[v][7])[4:] == str(np.datetime64(target_dt).astype('datetime64[s]'))[4:]
    c['delta_times'] = times                 # the records keep the edge inputs: only the stamps move
    return c
