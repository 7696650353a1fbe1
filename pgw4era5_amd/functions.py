"""
Host-side mirror of the reference's `functions.py` numerical API, backed by the HIP library.

Every function keeps the reference's name, argument order and error behaviour
(reference functions.py line ranges are cited per function) and runs on the GPU through the
C-ABI in include/pgw_hip.h.  There is no CPU implementation behind these names.

Accepted array kinds, everywhere a field is expected:
  * `numpy.ndarray` (float32/float64)      -> copied to the device, result returned as ndarray
  * `pgw4era5_amd.device.DeviceArray`      -> used in place, result stays on the device
  * labelled arrays (`pgw4era5_amd.ncio.Field`, or any object with `.values`, `.dims`,
    `.coords`)                             -> like ndarray, result re-wrapped with the labels
(`operands.py` holds these rules.)  4-D fields are C-order `(time, level, lat, lon)`.
"""
import ctypes as C
import datetime
import os

import numpy as np

from ._lib import _dp, _ip, _vpp, check_nplev
from .constants import CON_G, CON_RD, CON_MW_MD   # noqa: F401  (re-exported like the reference)
from .device import DeviceArray, default_context, dtype_tag, ptr
from .operands import (F64, aligned, check_extrapolate, common_dtype, dev, dev_own, fit, float_dtype, is_labelled, out_like,
                       raw, shape4)
from .settings import (                      # noqa: F401
    i_debug, i_use_xesmf_regridding, file_name_bases,
    TIME_ERA, LEV_ERA, HLEV_ERA, LON_ERA, LAT_ERA,
    TIME_GCM, PLEV_GCM, LON_GCM, LAT_GCM, LON_GCM_OCEAN, LAT_GCM_OCEAN,
)


# ------------------------------------------------------------------------------- dtype flow
# per function of settings.function_dtype_flow = 'reference': (operands that go to the device in their own dtype, operands
# that must be float64, result).  The result is 'promote' (numpy's promoted type of all operands), the name of the operand
# whose dtype it takes, 'float64', or a tuple of those for a function with several results.
_FLOW_RULES = {
    'specific_humidity_to_vapor_pressure': (('hus', 'pa'), (), 'promote'),                       # functions.py:58-64
    'vapor_pressure_to_specific_humidity': (('vapp', 'pa'), (), 'promote'),                      # :66-72
    'saturation_vapor_pressure_water_or_ice': (('ta',), (), 'ta'),                               # :74-89 (pa is unused)
    'saturation_vapor_pressure_water_and_ice': (('ta',), (), 'ta'),                              # :91-105
    'specific_to_relative_humidity': (('hus', 'pa', 'ta'), (), 'promote'),                       # :107-116
    'relative_to_specific_humidity': (('hur', 'pa', 'ta'), (), 'promote'),                       # :118-125
    'integ_geopot': (('zgs', 'ta', 'hus'), ('pa_hl', 'p_ref'), 'float64'),                       # :128-189
    'interp_logp_4d': (('var',), ('source_P', 'targ_P'), 'float64'),                             # :434-477
    'interp_1d_for_timelatlon': (('orig_array',), ('src_p', 'targ_p'), 'float64'),               # :479-508
    'interp_extrap_1d': (('src_y',), ('src_x', 'targ_x'), 'float64'),                            # :511-580
    'replace_delta_sfc': (('delta', 'delta_sfc', 'ps_hist'), ('source_P',), ('float64', 'delta')),   # :343-366
    'vert_interp_delta': (('delta', 'delta_sfc', 'ps_hist', 'add_to'), ('target_P',), 'float64'),    # :369-431
    'time_lerp': (('v_before', 'v_after'), (), 'float64'),                                       # :288-292
    'integrate_tos': (('tos_field', 'ts_field', 'land_frac', 'ice_frac'), (), 'float64'),        # :1145-1186
}


def _check_flow(value):
    if value not in ('common', 'reference'):
        raise ValueError("settings.function_dtype_flow must be 'common' or 'reference', got %r" % (value,))
    return value


def _flow():
    """settings.function_dtype_flow, read at call time."""
    from . import settings as S
    return _check_flow(S.function_dtype_flow)


def reference_dtype_flow(function, **dtypes):
    """What settings.function_dtype_flow = 'reference' does with operands of the given dtypes, without touching a GPU:
    `(tags, result)` - `tags[operand]` is the C-ABI dtype tag (`_lib.PGW_F32` / `PGW_F64`) the operand is handed over with, in
    its own dtype; `result` the dtype the reference returns (a tuple of dtypes for replace_delta_sfc: P, D).  Operands that
    are None (an absent delta_sfc, a scalar p_ref) are left out.  A float32 array where the reference would then take a
    float32 logarithm (pa_hl, a p_ref field, the pressures / abscissae of the interpolations) raises NotImplementedError:
    that flow is not built, and it is not computed in float64 under the name 'reference'."""
    try:
        own, need64, result = _FLOW_RULES[function]
    except KeyError:
        raise ValueError('%s has no reference dtype flow' % function) from None
    unknown = set(dtypes) - set(own) - set(need64)
    if unknown:
        raise TypeError('%s: unknown operand(s) %s' % (function, sorted(unknown)))
    given = {k: float_dtype(v) for k, v in dtypes.items() if v is not None}
    for name in need64:
        if name in given and given[name] != F64:
            raise NotImplementedError(
                "%s: a float32 `%s` would make the reference take its logarithm in float32; that flow is not built - use "
                "settings.function_dtype_flow = 'common' (or hand `%s` over as float64)" % (function, name, name))
    tags = {k: dtype_tag(v) for k, v in given.items()}

    def res(rule):
        if rule == 'float64':
            return F64
        if rule == 'promote':
            have = [given[k] for k in own if k in given]
            return np.result_type(*have) if have else None
        return given.get(rule)
    return tags, (tuple(res(r) for r in result) if isinstance(result, tuple) else res(result))


class OperandPlan:
    """How the named operands `xs` of one call of `function` reach its kernel, decided once and before anything is uploaded:
    `reference` - the call runs under settings.function_dtype_flow = 'reference' (read here, and only for a function of
    `_FLOW_RULES`): every operand goes in its own dtype, as `reference_dtype_flow` says (its NotImplementedError is raised
    here); otherwise every operand is cast to one dtype - `common` where the entry fixes it, else `common_dtype` of the
    operands.  `result` is the dtype of the result (a pair for replace_delta_sfc).  Operands that are None stay None."""

    def __init__(self, ctx, function, common=None, **xs):
        self.ctx, self.xs = ctx, xs
        self.reference = function in _FLOW_RULES and _flow() == 'reference'
        if self.reference:
            self.tags, self.result = reference_dtype_flow(
                function, **{n: None if x is None else raw(x).dtype for n, x in xs.items()})
        else:
            self.dtype = common_dtype(*xs.values()) if common is None else np.dtype(common)
            rule = _FLOW_RULES.get(function)
            self.result = (self.dtype,) * len(rule[2]) if rule and isinstance(rule[2], tuple) else self.dtype

    def dev(self, name, shape=None):
        """The operand on the device (viewed / uploaded as `shape`): in its own dtype, or cast to the common one - where a
        DeviceArray of another dtype is a TypeError."""
        if self.reference:
            return dev_own(self.ctx, self.xs[name], shape)
        return dev(self.ctx, self.xs[name], self.dtype, shape)

    def tag(self, name):
        """C-ABI dtype tag of the operand: its own (0 when it is absent), or the one common tag."""
        return self.tags.get(name, 0) if self.reference else dtype_tag(self.dtype)


# ------------------------------------------------------------------------------- humidity
def _humidity(function, which, **xs):
    """Entry `which` of the humidity family on the operands `xs`: the reference's argument names, the leading operand first
    (the others are aligned and broadcast to it, and the result comes back in its kind).  `xs` keeps the caller's keyword
    order, which is the C argument order.  C entries reached: `pgw_humidity_mixed` (reference flow, every `which`),
    `pgw_humidity_leaf` (which 0-4: the one- and two-operand leaves), and for the two three-operand wrappers (which 5, 6)
    the entry of their own name, `pgw_specific_to_relative_humidity` / `pgw_relative_to_specific_humidity`."""
    ctx = default_context()
    names = list(xs)
    lead = xs[names[0]]
    shp = raw(lead).shape
    ops = OperandPlan(ctx, function, **{n: fit(aligned(x, lead), shp, n) if n != names[0] else x for n, x in xs.items()})
    d = [ops.dev(n) for n in names] + [None, None]
    out = ctx.empty(shp, ops.result)
    if ops.reference:
        t = [ops.tag(n) for n in names] + [0, 0]
        rc = ctx.lib.pgw_humidity_mixed(ctx.handle, which, t[0], t[1], t[2], out.size, d[0].ptr, ptr(d[1]), ptr(d[2]), out.ptr)
    elif which < 5:
        rc = ctx.lib.pgw_humidity_leaf(ctx.handle, ops.tag(names[0]), which, out.size, d[0].ptr, ptr(d[1]), out.ptr)
    else:
        rc = getattr(ctx.lib, 'pgw_' + function)(ctx.handle, ops.tag(names[0]), out.size, d[0].ptr, d[1].ptr, d[2].ptr, out.ptr)
    ctx._check(rc)
    return out_like(out, lead)


def specific_to_relative_humidity(hus, pa, ta):
    """RH [%] from specific humidity (IFS 7.92/7.93).  reference functions.py:107-116."""
    return _humidity('specific_to_relative_humidity', 5, hus=hus, pa=pa, ta=ta)


def relative_to_specific_humidity(hur, pa, ta):
    """Specific humidity from RH [%].  reference functions.py:118-125."""
    return _humidity('relative_to_specific_humidity', 6, hur=hur, pa=pa, ta=ta)


def specific_humidity_to_vapor_pressure(hus, pa):
    """e = hus * pa / (0.622 + 0.378 * hus).  reference functions.py:58-64."""
    return _humidity('specific_humidity_to_vapor_pressure', 0, hus=hus, pa=pa)


def vapor_pressure_to_specific_humidity(vapp, pa):
    """hus = 0.622 * vapp / (pa - 0.378 * vapp).  reference functions.py:66-72."""
    return _humidity('vapor_pressure_to_specific_humidity', 1, vapp=vapp, pa=pa)


def saturation_vapor_pressure_water_or_ice(pa, ta, water=True):
    """IFS (7.93) saturation vapour pressure over water or over ice; `pa` is unused, as in the reference (functions.py:74-89)."""
    return _humidity('saturation_vapor_pressure_water_or_ice', 2 if water else 3, ta=ta)


def saturation_vapor_pressure_water_and_ice(pa, ta):
    """IFS (7.92) mixed-phase saturation vapour pressure.  reference functions.py:91-105."""
    return _humidity('saturation_vapor_pressure_water_and_ice', 4, ta=ta)


def dt64_to_dt(dt64):
    """numpy datetime64 -> python datetime (UTC).  reference functions.py:38-51."""
    timestamp = (np.datetime64(dt64, 's') - np.datetime64('1970-01-01T00:00:00')) / np.timedelta64(1, 's')
    return datetime.datetime.utcfromtimestamp(float(timestamp))


# ------------------------------------------------------------------------------- pressure
def hybrid_pressure(ak, bk, ps, akm=None, bkm=None):
    """pa_hl = ak + ps*bk, pa = akm + ps*bkm  (reference step_03_apply_to_era.py:64-88,196-199;
    this is what BASELINE.json calls "integ_pressure").  ps (time, lat, lon) -> (pa_hl, pa)."""
    ctx = default_context()
    ctx.set_levels(ak, bk, akm, bkm)
    ops = OperandPlan(ctx, 'hybrid_pressure', ps=ps)
    s = raw(ps).shape
    if len(s) != 3:
        raise ValueError('ps must be (time, lat, lon)')
    nt, ncol, n = s[0], s[1] * s[2], ctx.nlev
    dps = ops.dev('ps')
    # the kernel's two write streams in different stretches of the card's memory when the context places its level arrays
    # (settings.placement; Context.level_array falls back to plain memory): 0.34 instead of 0.41 ms at 0.25 deg L137
    pa_hl = ctx.level_array((nt, n + 1, s[1], s[2]), ops.result, cls=0)
    pa = ctx.level_array((nt, n, s[1], s[2]), ops.result, cls=1)
    ctx._check(ctx.lib.pgw_pressure_levels(ctx.handle, ops.tag('ps'), nt, ncol, dps.ptr, pa_hl.ptr, pa.ptr))
    if isinstance(ps, DeviceArray):
        return pa_hl, pa
    return pa_hl.numpy(), pa.numpy()


# ------------------------------------------------------------------------------- integ_geopot
def integ_geopot(pa_hl, zgs, ta, hus, level1, p_ref, full_column=True):
    """Geopotential at p_ref by hydrostatic integration from the surface.
    reference functions.py:128-189.  `level1` = half-level labels (its length must be N+1).
    p_ref: scalar or (time, lat, lon) field.  Returns (time, lat, lon).
    Under settings.function_dtype_flow = 'reference': phi_hl in the dtype of zgs, tav in the promoted dtype of (ta, hus),
    float64 pressures, float64 result."""
    ctx = default_context()
    hus = aligned(hus, ta)
    s = shape4(pa_hl)
    st = shape4(ta)
    if len(level1) != s[1] or st[1] != s[1] - 1 or shape4(hus) != st:
        raise ValueError('level dimensions are inconsistent')
    nt, n, ncol, s3 = s[0], st[1], s[2] * s[3], (s[0], s[2], s[3])
    ta_, hus_ = fit(ta, (nt, n, s[2], s[3]), 'ta'), fit(hus, (nt, n, s[2], s[3]), 'hus')
    pr = raw(p_ref) if not np.isscalar(p_ref) else None
    is_field = pr is not None and (isinstance(pr, DeviceArray) or pr.ndim > 0)
    # a p_ref field follows the common dtype of the other four, it has no say in it
    ops = OperandPlan(ctx, 'integ_geopot', common=common_dtype(pa_hl, zgs, ta, hus),
                      pa_hl=pa_hl, zgs=zgs, ta=ta_, hus=hus_, p_ref=p_ref if is_field else None)
    d_p, d_z, d_t, d_q, d_ref = ops.dev('pa_hl'), ops.dev('zgs', s3), ops.dev('ta'), ops.dev('hus'), ops.dev('p_ref', s3)
    out = ctx.empty(s3, ops.result)
    tail = (nt, n, ncol, d_p.ptr, d_z.ptr, d_t.ptr, d_q.ptr, 0.0 if is_field else float(p_ref), ptr(d_ref), out.ptr,
            1 if full_column else 0)
    if ops.reference:
        rc = ctx.lib.pgw_integ_geopot_mixed(ctx.handle, ops.tag('pa_hl'), ops.tag('zgs'), ops.tag('ta'), ops.tag('hus'), *tail)
    else:
        rc = ctx.lib.pgw_integ_geopot(ctx.handle, ops.tag('pa_hl'), *tail)
    ctx._check(rc)
    return out_like(out, zgs)


# ------------------------------------------------------------------------------- interpolation
def _interp_logp(ops, var, targ, dims, d_v, d_s, d_t, mode, is_logp, out):
    """Status of `pgw_interp_logp_4d` (`_mixed` in the reference flow, which takes the tags of the operands named `var` and
    `targ`) for dims = (nt, S, N, ncol)."""
    ctx = ops.ctx
    tail = dims + (d_v.ptr, d_s.ptr, d_t.ptr, mode, is_logp, out.ptr)
    if ops.reference:
        return ctx.lib.pgw_interp_logp_4d_mixed(ctx.handle, ops.tag(var), ops.tag(targ), *tail)
    return ctx.lib.pgw_interp_logp_4d(ctx.handle, ops.tag(var), *tail)


def interp_logp_4d(var, source_P, targ_P, extrapolate='off', time_key=None, lat_key=None, lon_key=None):
    """Column-wise linear interpolation in ln(p).  reference functions.py:434-477.
    var, source_P (time, S, lat, lon); targ_P (time, N, lat, lon) -> (time, N, lat, lon)."""
    mode = check_extrapolate(extrapolate)
    sv, ss, st = shape4(var), shape4(source_P), shape4(targ_P)
    if (sv[0] != ss[0]) or (sv[0] != st[0]):
        raise ValueError('Time dimension of input files is inconsistent!')
    if (sv[2] != ss[2]) or (sv[2] != st[2]):
        raise ValueError('Lat dimension of input files is inconsistent!')
    if (sv[3] != ss[3]) or (sv[3] != st[3]):
        raise ValueError('Lon dimension of input files is inconsistent!')
    if sv[1] != ss[1]:
        raise ValueError('Level dimension of var and source_P is inconsistent!')
    ctx = default_context()
    ops = OperandPlan(ctx, 'interp_logp_4d', var=var, source_P=source_P, targ_P=targ_P)
    d_v, d_s, d_t = ops.dev('var'), ops.dev('source_P'), ops.dev('targ_P')
    out = ctx.empty(st, ops.result)
    ctx._check(_interp_logp(ops, 'var', 'targ_P', (st[0], sv[1], st[1], st[2] * st[3]), d_v, d_s, d_t, mode, 0, out))
    return out_like(out, targ_P)


def interp_1d_for_timelatlon(orig_array, src_p, targ_p, interp_array, ntime, nlat, nlon, extrapolate):
    """reference functions.py:479-508: inputs already hold ln(p); fills `interp_array` in place."""
    mode = check_extrapolate(extrapolate)
    ctx = default_context()
    ops = OperandPlan(ctx, 'interp_1d_for_timelatlon', common=F64, orig_array=orig_array, src_p=src_p, targ_p=targ_p)
    d_v, d_s, d_t = ops.dev('orig_array'), ops.dev('src_p'), ops.dev('targ_p')
    out = ctx.empty(d_t.shape, ops.result)
    ctx._check(_interp_logp(ops, 'orig_array', 'targ_p', (ntime, d_s.shape[1], d_t.shape[1], nlat * nlon), d_v, d_s, d_t, mode, 1, out))
    interp_array[...] = out.numpy()


def interp_extrap_1d(src_x, src_y, targ_x, extrapolate):
    """reference functions.py:511-580 for one column (abscissae as given, e.g. ln p)."""
    mode = check_extrapolate(extrapolate)
    ctx = default_context()
    S, N = len(src_x), len(targ_x)
    ops = OperandPlan(ctx, 'interp_extrap_1d', common=F64, src_x=src_x, src_y=src_y, targ_x=targ_x)
    d_s, d_v, d_t = ops.dev('src_x', (1, S, 1, 1)), ops.dev('src_y', (1, S, 1, 1)), ops.dev('targ_x', (1, N, 1, 1))
    out = ctx.empty((1, N, 1, 1), ops.result)
    rc = _interp_logp(ops, 'src_y', 'targ_x', (1, S, N, 1), d_v, d_s, d_t, mode, 1, out)
    # the 1-D function has no ascending pre-check (that lives in interp_1d_for_timelatlon)
    ctx._check(0 if rc in (10, 11) else rc)
    return out.numpy().reshape(N)


# ------------------------------------------------------------------------------- deltas
def time_lerp(v_before, v_after, x_hi, x_new):
    """(v_after - v_before)/x_hi * x_new + v_before: the arithmetic under load_delta's
    `.interp(time=...)` (reference functions.py:288-292; scipy interp1d linear)."""
    ctx = default_context()
    ops = OperandPlan(ctx, 'time_lerp', v_before=v_before, v_after=fit(v_after, raw(v_before).shape, 'v_after'))
    d_b, d_a = ops.dev('v_before'), ops.dev('v_after')
    out = ctx.empty(d_b.shape, ops.result)
    tail = (out.size, d_b.ptr, d_a.ptr, float(x_hi), float(x_new), out.ptr)
    if ops.reference:
        rc = ctx.lib.pgw_time_lerp_mixed(ctx.handle, ops.tag('v_before'), ops.tag('v_after'), *tail)
    else:
        rc = ctx.lib.pgw_time_lerp(ctx.handle, ops.tag('v_before'), *tail)
    ctx._check(rc)
    return out_like(out, v_before)


def replace_delta_sfc(source_P, ps_hist, delta, delta_sfc):
    """reference functions.py:343-366 for one ascending-pressure column."""
    ctx = default_context()
    ops = OperandPlan(ctx, 'replace_delta_sfc', common=F64, source_P=source_P, delta=delta, delta_sfc=delta_sfc, ps_hist=ps_hist)
    if ops.reference:                                       # a column without len() (DeviceArray, Field) fails here in this
        len(source_P)                                       # flow and in the cast below in the other: each keeps its own
    P = np.ascontiguousarray(source_P, dtype=F64)           # read on the host; float64 in both flows
    S = len(P)
    check_nplev(S, 1, 'len(source_P)')
    d_d, d_s, d_p = ops.dev('delta', (1, S, 1)), ops.dev('delta_sfc', (1, 1)), ops.dev('ps_hist', (1, 1))
    oP, oD = (ctx.empty((1, S, 1), dt) for dt in ops.result)
    tail = (1, S, 1, P.ctypes.data_as(_dp), d_d.ptr, d_s.ptr, d_p.ptr, oP.ptr, oD.ptr)
    if ops.reference:
        rc = ctx.lib.pgw_replace_delta_sfc_mixed(ctx.handle, ops.tag('delta'), ops.tag('delta_sfc'), ops.tag('ps_hist'), *tail)
    else:
        rc = ctx.lib.pgw_replace_delta_sfc(ctx.handle, ops.tag('delta'), *tail)
    ctx._check(rc)
    return oP.numpy().reshape(S), oD.numpy().reshape(S)


def _plev_of(delta, plev):
    if plev is not None:
        return np.ascontiguousarray(plev, dtype=np.float64)
    if is_labelled(delta) and PLEV_GCM in getattr(delta, 'coords', {}):
        return np.ascontiguousarray(delta.coords[PLEV_GCM], dtype=np.float64)
    raise ValueError('vert_interp_delta needs the plev coordinate (labelled delta or plev=...)')


def vert_interp_delta(delta, target_P, delta_sfc=None, ps_hist=None, ignore_top_pressure_error=False,
                      plev=None, add_to=None, _bracket=None):
    """Vertical interpolation of a climate delta onto model levels, with the surface delta
    inserted at the HIST surface pressure.  reference functions.py:369-431 (+ :343-366).
    delta (time, plev, lat, lon) in the file's plev order (reversed inside like :383-384);
    target_P (time, N, lat, lon); delta_sfc, ps_hist (time, lat, lon) or None."""
    ctx = default_context()
    pl = _plev_of(delta, plev)
    sd, st = shape4(delta), shape4(target_P)
    if sd[0] != st[0] or sd[2:] != st[2:]:
        raise ValueError()
    if (delta_sfc is None) != (ps_hist is None):
        raise ValueError('delta_sfc and ps_hist must be given together')
    nt, S, ncol, N, s3 = sd[0], sd[1], sd[2] * sd[3], st[1], (sd[0], sd[2], sd[3])
    check_nplev(S)                                          # 2 to 128 levels, before anything reaches the device
    # the common dtype is decided on the caller's add_to: `fit` keeps an operand's dtype, so the fitted one decides the same
    ops = OperandPlan(ctx, 'vert_interp_delta', delta=delta, target_P=target_P, delta_sfc=delta_sfc, ps_hist=ps_hist,
                      add_to=None if add_to is None else fit(add_to, st, 'add_to'))
    d_d, d_t, d_s, d_p, d_add = ops.dev('delta'), ops.dev('target_P'), ops.dev('delta_sfc', s3), ops.dev('ps_hist', s3), ops.dev('add_to')
    out = ctx.empty(st, ops.result)
    top = 1 if ignore_top_pressure_error else 0
    if ops.reference:
        rc = ctx.lib.pgw_vert_interp_delta_mixed(
            ctx.handle, ops.tag('delta'), ops.tag('delta_sfc'), ops.tag('ps_hist'), ops.tag('target_P'), ops.tag('add_to'),
            nt, S, N, ncol, pl.ctypes.data_as(_dp), d_d.ptr, ptr(d_s), ptr(d_p), d_t.ptr, top, ptr(d_add), out.ptr)
    else:
        rc = ctx.lib.pgw_vert_interp_delta(
            ctx.handle, ops.tag('delta'), nt, S, N, ncol, pl.ctypes.data_as(_dp),
            d_d.ptr, None, 0.0, 0.0, ptr(d_s), None, ptr(d_p), None, d_t.ptr, None, top, ptr(d_add), out.ptr)
    ctx._check(rc)
    return out_like(out, target_P)


def determine_p_ref(p_min_era, p_min_pgw, p_ref_opts, p_ref_last=None):
    """reference functions.py:583-598 (scalar control logic; host side like the reference)."""
    for p in p_ref_opts:
        if (p_min_era > p) & (p_min_pgw > p):
            if p_ref_last is None:
                return p
            return min(p, p_ref_last)


def integrate_tos(tos_field, ts_field, land_frac, ice_frac):
    """Blend SST and skin-temperature deltas by land + sea-ice fraction.
    reference functions.py:1145-1186."""
    ctx = default_context()
    names = ('tos_field', 'ts_field', 'land_frac', 'ice_frac')
    ops = OperandPlan(ctx, 'integrate_tos', **dict(zip(names, (tos_field, ts_field, land_frac, ice_frac))))
    d = [ops.dev(n) for n in names]
    out = ctx.empty(raw(tos_field).shape, ops.result)
    tail = (out.size, d[0].ptr, d[1].ptr, d[2].ptr, d[3].ptr, out.ptr)
    if ops.reference:
        rc = ctx.lib.pgw_integrate_tos_mixed(ctx.handle, *[ops.tag(n) for n in names], *tail)
    else:
        rc = ctx.lib.pgw_integrate_tos(ctx.handle, ops.tag(names[0]), *tail)
    ctx._check(rc)
    return out_like(out, tos_field)


# ------------------------------------------------------------------------------- ps loop
def adjust_ps_loop(ak, bk, PS, FIS, T, QV, ta_pgw, hur_pgw, dzg_pref, akm=None, bkm=None,
                   p_ref=None, adj_factor=None, thresh=None, max_n_iter=None, want_hus=True):
    """The iterative surface-pressure adjustment, reference step_03_apply_to_era.py:182-319
    (fixed p_ref).  Returns dict(ps_pgw, hus_pgw, n_iter, max_err).  Raises the reference's
    ValueError on non-convergence."""
    from . import settings as S
    p_ref = S.p_ref_inp if p_ref is None else p_ref
    adj_factor = S.adj_factor if adj_factor is None else adj_factor
    thresh = S.thresh_phi_ref_max_error if thresh is None else thresh
    max_n_iter = S.max_n_iter if max_n_iter is None else max_n_iter
    ctx = default_context()
    ctx.set_levels(ak, bk, akm, bkm)
    s = shape4(ta_pgw)
    ops = OperandPlan(ctx, 'adjust_ps_loop', PS=PS, FIS=FIS, T=T, QV=QV, ta=ta_pgw, hur=hur_pgw, dzg=dzg_pref)
    nt, ncol = s[0], s[2] * s[3]
    s3 = (nt, s[2], s[3])
    d = {n: ops.dev(n, s3 if n in ('PS', 'FIS', 'dzg') else None) for n in ('PS', 'FIS', 'T', 'QV', 'ta', 'hur', 'dzg')}
    ps_out = ctx.empty(s3, ops.result)
    hus_out = ctx.empty(s, ops.result) if want_hus else None
    n_iter = C.c_int(0)
    hist = (C.c_double * int(max_n_iter))()
    rc = ctx.lib.pgw_adjust_ps_loop(ctx.handle, ops.tag('ta'), nt, ncol, d['PS'].ptr, d['FIS'].ptr, d['T'].ptr,
                                    d['QV'].ptr, d['ta'].ptr, d['hur'].ptr, d['dzg'].ptr, float(p_ref),
                                    float(adj_factor), float(thresh), int(max_n_iter), ps_out.ptr, ptr(hus_out),
                                    C.byref(n_iter), hist)
    ctx._check(rc)
    res = dict(n_iter=n_iter.value, max_err=[hist[i] for i in range(n_iter.value)],
               levels_touched=int(ctx.lib.pgw_last_levels_touched(ctx.handle)))
    if isinstance(ta_pgw, DeviceArray):
        res.update(ps_pgw=ps_out, hus_pgw=hus_out)
    else:
        res.update(ps_pgw=ps_out.numpy(), hus_pgw=hus_out.numpy() if want_hus else None)
    return res


# ------------------------------------------------------------------------------- hydrostatic check
# How two states meet in `pgw_geopot_on_plev`: 0 = both in one walk of the column, 1 = one walk each in the same launch.
# The same bits.  1 is the form that beat the composed calls for float64 AND float32 level arrays.
GEOPOT_PLEV_FORM = 1


def check_plev(plev, most=64):
    """The level list of the hydrostatic check as a float64 vector: 1 to 64 finite pressures above 1e-4 Pa, the guard value
    of reference functions.py:135 (ValueError otherwise, before anything reaches the device).  `most`: the capacity of
    the entry that takes the list (the delta check follows the delta axes: 128)."""
    p = np.ascontiguousarray(raw(plev), dtype=np.float64)
    if p.ndim != 1 or not 1 <= p.size <= most:
        raise ValueError('plev must be a vector of 1 to %d levels, got shape %s' % (most, p.shape))
    if not np.all(np.isfinite(p)):
        raise ValueError('plev must be finite')
    if not np.all(p > 0.0001):
        raise ValueError('plev must be greater than 1e-4 Pa')
    return p


def _geopot_plev(states, zgs, ak, bk, plev, dzg, counts, form):
    p = check_plev(plev)
    ak_, bk_ = np.asarray(raw(ak), dtype=np.float64), np.asarray(raw(bk), dtype=np.float64)
    if ak_.ndim != 1 or ak_.shape != bk_.shape or ak_.size < 2:
        raise ValueError('ak and bk must be vectors of one length (nlev + 1)')
    s3 = tuple(raw(zgs).shape)
    if len(s3) != 3:
        raise ValueError('zgs must be (time, lat, lon), got shape %s' % (s3,))
    nlev = ak_.size - 1
    for i, (ps, ta, hus) in enumerate(states):
        st = shape4(ta)
        lab = 'state %s' % 'ab'[i]
        if shape4(hus) != st:
            raise ValueError('%s: ta %s and hus %s differ in shape' % (lab, st, shape4(hus)))
        if (st[0], st[2], st[3]) != s3 or tuple(raw(ps).shape) != s3:
            raise ValueError('%s: ps %s / ta %s do not lie on the grid %s of zgs' % (lab, tuple(raw(ps).shape), st, s3))
        if st[1] != nlev:
            raise ValueError('%s: %d levels, but ak and bk describe %d' % (lab, st[1], nlev))
    zg = None
    if dzg is not None:
        zb, za, x_hi, x_new = dzg if isinstance(dzg, tuple) else (dzg, None, 0.0, 0.0)
        sz = (s3[0], p.size, s3[1], s3[2])
        if shape4(zb) != sz or (za is not None and shape4(za) != sz):
            raise ValueError('dzg must be (time, plev, lat, lon) = %s' % (sz,))
        if za is None and float(x_hi) != 0.0:
            raise ValueError('dzg: the record after the instant is needed unless x_hi is 0')
        zg = (zb, za, float(x_hi), float(x_new))
    if form not in (None, 0, 1):
        raise ValueError('form must be 0 or 1')
    # nothing has touched the device up to here
    ctx = default_context()
    ctx.set_levels(ak_, bk_)
    dt2 = common_dtype(zgs, *[s[0] for s in states])
    d_z = dev(ctx, zgs, dt2, s3)
    d_states, tags = [], []
    for ps, ta, hus in states:
        dtl = common_dtype(ta, hus)
        d_states.append((dev(ctx, ps, dt2, s3), dev(ctx, ta, dtl), dev(ctx, hus, dtl)))
        tags.append(dtype_tag(dtl))
    if len(states) == 1:
        d_states.append((None, None, None))
        tags.append(0)
    tz, d_zb, d_za, x_hi, x_new = 0, None, None, 0.0, 0.0
    if zg is not None:
        dtz = common_dtype(zg[0], zg[1])
        tz, d_zb, d_za, x_hi, x_new = dtype_tag(dtz), dev(ctx, zg[0], dtz), dev(ctx, zg[1], dtz), zg[2], zg[3]
    out = ctx.empty((s3[0], p.size, s3[1], s3[2]), F64)
    nan = (C.c_longlong * p.size)()
    (pa, ta_a, qa), (pb, ta_b, qb) = d_states
    ctx._check(ctx.lib.pgw_geopot_on_plev(
        ctx.handle, dtype_tag(dt2), tags[0], tags[1], s3[0], p.size, s3[1] * s3[2], p.ctypes.data_as(_dp), d_z.ptr,
        pa.ptr, ta_a.ptr, qa.ptr, ptr(pb), ptr(ta_b), ptr(qb), tz, ptr(d_zb), ptr(d_za), x_hi, x_new, CON_G,
        int(GEOPOT_PLEV_FORM if form is None else form), out.ptr, nan))
    res = out if isinstance(raw(states[0][1]), DeviceArray) else out.numpy()
    return (res, np.array(nan[:], dtype=np.int64)) if counts else res


def geopot_on_plev(ps, zgs, ta, hus, ak, bk, plev, counts=False):
    """Geopotential of one state on every pressure of `plev`: reference functions.py:128-189 (`integ_geopot`) with
    pa_hl = ak + ps * bk evaluated at p_ref = plev[i] for all i in one walk of the columns.  ps, zgs (time, lat, lon);
    ta, hus (time, N, lat, lon); returns (time, plev, lat, lon) float64 in the order of `plev` - a DeviceArray for
    DeviceArray input, an ndarray otherwise.  NaN where the level lies below the column's surface half level (the reference
    raises there, :162-165).  float64 arithmetic on the stored values; `counts=True` also returns the NaN count per level.
    ValueError for inconsistent shapes or level counts and for a `plev` that is not finite and above 1e-4 Pa."""
    return _geopot_plev([(ps, ta, hus)], zgs, ak, bk, plev, None, counts, None)


def geopot_change_on_plev(ps_a, ta_a, hus_a, ps_b, ta_b, hus_b, zgs, ak, bk, plev, dzg=None, counts=False, form=None):
    """phi_b - phi_a of two states that share zgs and the coefficients (`geopot_on_plev` of each, one launch), the loop's
    `phi_ref_pgw - phi_ref_era` (reference step_03_apply_to_era.py:289) on every level of `plev`.  With `dzg` - the zg delta
    (time, plev, lat, lon) in the order of `plev`, or `(record_before, record_after, x_hi, x_new)` for the time
    interpolation of `load_delta` (functions.py:288-292) - the result is phi_error = (phi_b - phi_a) - g * dzg (step_03:298).
    NaN where either state is NaN.  The level arrays of each state keep their own dtype; the surface fields share one."""
    return _geopot_plev([(ps_a, ta_a, hus_a), (ps_b, ta_b, hus_b)], zgs, ak, bk, plev, dzg, counts, form)


def level_stats(x):
    """Per row of x (nrow, ncol) float64, NaN skipped: dict(count, sum, sumsq, maxabs) as host vectors (`pgw_level_stats`);
    two calls give the same bits."""
    r = raw(x)
    if len(r.shape) != 2 or r.shape[0] < 1 or r.shape[1] < 1:
        raise ValueError('level_stats takes a non-empty (nrow, ncol) array, got shape %s' % (tuple(r.shape),))
    ctx = default_context()
    d = dev(ctx, x, F64)
    n = r.shape[0]
    cnt, s, q, m = (C.c_longlong * n)(), (C.c_double * n)(), (C.c_double * n)(), (C.c_double * n)()
    ctx._check(ctx.lib.pgw_level_stats(ctx.handle, n, r.shape[1], d.ptr, cnt, s, q, m))
    return dict(count=np.array(cnt[:], dtype=np.int64), sum=np.array(s[:]), sumsq=np.array(q[:]), maxabs=np.array(m[:]))


# ------------------------------------------------------------------------------- delta check
STATE_PLEV_VARS = ('ta', 'hur', 'ua', 'va')              # variable order of `pgw_state_on_plev`, everywhere


def _state_plev(states, ak, bk, plev, deltas):
    p = check_plev(plev, most=128)
    ak_, bk_ = np.asarray(raw(ak), dtype=np.float64), np.asarray(raw(bk), dtype=np.float64)
    if ak_.ndim != 1 or ak_.shape != bk_.shape or ak_.size < 2:
        raise ValueError('ak and bk must be vectors of one length (nlev + 1)')
    nlev = ak_.size - 1
    s3 = tuple(raw(states[0][0]).shape)
    if len(s3) != 3:
        raise ValueError('ps must be (time, lat, lon), got shape %s' % (s3,))
    for i, (ps, ta, hus, ua, va) in enumerate(states):
        st = shape4(ta)
        lab = 'state %s' % 'ab'[i]
        for name, x in (('hus', hus), ('ua', ua), ('va', va)):
            if shape4(x) != st:
                raise ValueError('%s: ta %s and %s %s differ in shape' % (lab, st, name, shape4(x)))
        if (st[0], st[2], st[3]) != s3 or tuple(raw(ps).shape) != s3:
            raise ValueError('%s: ps %s / ta %s do not lie on the grid %s' % (lab, tuple(raw(ps).shape), st, s3))
        if st[1] != nlev:
            raise ValueError('%s: %d levels, but ak and bk describe %d' % (lab, st[1], nlev))
    recs = None
    if deltas is not None:
        if len(states) != 2:
            raise ValueError('deltas need two states')
        s4, recs = (s3[0], p.size, s3[1], s3[2]), []
        for name in STATE_PLEV_VARS + ('ps_hist',):
            if name not in deltas:
                raise ValueError('deltas: %s is missing (needed: ta, hur, ua, va, ps_hist)' % name)
            b, a, x_hi, x_new = deltas[name]
            want = s3 if name == 'ps_hist' else s4
            for r in (b, a):
                if r is None or int(np.prod(raw(r).shape, dtype=np.int64)) != int(np.prod(want, dtype=np.int64)) or \
                        tuple(raw(r).shape)[-2:] != want[-2:]:
                    raise ValueError('deltas: the records of %s must be %s, got %s' % (name, want, None if r is None else tuple(raw(r).shape)))
            recs.append((b, a, float(x_hi), float(x_new), want))
    # nothing has touched the device up to here
    ctx = default_context()
    ctx.set_levels(ak_, bk_)
    dt2 = common_dtype(*[s[0] for s in states])
    d_states, tags, held = [], [], []
    for st in states:
        dtl = common_dtype(*st[1:])
        d = [dev(ctx, st[0], dt2, s3)] + [dev(ctx, x, dtl) for x in st[1:]]
        d_states.append(d)
        tags.append(dtype_tag(dtl))
    if len(states) == 1:
        d_states.append([None] * 5)
        tags.append(0)
    shape = (4, s3[0], p.size, s3[1], s3[2])
    out = ctx.empty(shape, F64)
    err = None
    tdel, rb, ra, x_hi, x_new = 0, (C.c_void_p * 4)(), (C.c_void_p * 4)(), (C.c_double * 5)(), (C.c_double * 5)()
    psb = psa = None
    if recs is not None:
        dtd = common_dtype(*[r for rec in recs for r in rec[:2]])
        tdel = dtype_tag(dtd)
        for i, (b, a, xh, xn, want) in enumerate(recs):
            d_b, d_a = dev(ctx, b, dtd, want), dev(ctx, a, dtd, want)
            held += [d_b, d_a]
            x_hi[i], x_new[i] = xh, xn
            if i < 4:
                rb[i], ra[i] = d_b.ptr, d_a.ptr
            else:
                psb, psa = d_b, d_a
        err = ctx.empty(shape, F64)
    a_, b_ = d_states
    ctx._check(ctx.lib.pgw_state_on_plev(
        ctx.handle, dtype_tag(dt2), tags[0], tags[1], s3[0], p.size, s3[1] * s3[2], p.ctypes.data_as(_dp),
        *[x.ptr for x in a_], *[ptr(x) for x in b_], tdel, C.cast(rb, _vpp), C.cast(ra, _vpp), ptr(psb), ptr(psa), x_hi, x_new,
        out.ptr, ptr(err)))
    return out, err


def state_on_plev(ps, ta, hus, ua, va, ak, bk, plev):
    """T, RH, U, V of an ERA5-like state on every pressure of `plev` (`pgw_state_on_plev`): pa = akm + ps * bkm,
    RH = specific_to_relative_humidity(hus, pa, ta) (reference functions.py:107-116), each variable through
    interp_extrap_1d(ln pa, X, ln p, 'nan') (:511-580).  ps (time, H0, H1); ta, hus, ua, va (time, N, H0, H1), numpy arrays
    or DeviceArrays; returns a DeviceArray (4, time, plev, H0, H1) float64 in the order (ta, hur, ua, va), rows in the
    order of `plev` (1 to 128 levels).  NaN above the top and below the lowest full level.  float64 arithmetic on the
    stored values.  ValueError for inconsistent shapes or level counts and for a bad `plev`, before the device is touched."""
    return _state_plev([(ps, ta, hus, ua, va)], ak, bk, plev, None)[0]


def state_change_on_plev(ps_a, ta_a, hus_a, ua_a, va_a, ps_b, ta_b, hus_b, ua_b, va_b, ak, bk, plev, deltas=None):
    """`state_on_plev` of state b minus that of state a, in one launch: (change, None).  With `deltas` - a mapping of
    'ta', 'hur', 'ua', 'va' and 'ps_hist' to `(record_before, record_after, x_hi, x_new)` as `DeltaSet.pair` hands them
    out, the level records (time, plev, H0, H1) in the order of `plev` - also error = change - delta where plev < ps_hist,
    NaN elsewhere, delta and ps_hist interpolated in time like load_delta (functions.py:288-292), each on its own axis:
    (change, error).  Both are DeviceArrays (4, time, plev, H0, H1) float64."""
    return _state_plev([(ps_a, ta_a, hus_a, ua_a, va_a), (ps_b, ta_b, hus_b, ua_b, va_b)], ak, bk, plev, deltas)


# ------------------------------------------------------------------------------- postproc_cosmo
def _mean_add_plan(base, x, mask_values, out):
    """Shapes and dtypes of one `pgw_time_mean_add` call, checked before the device is touched: x is (nrec,) + S, base is S
    or S behind leading axes of length 1 (`T_CL(time=1, rlat, rlon)` meeting the squeezed mean of the reference).
    -> (nrec, n, S, mask vector)."""
    sx = tuple(raw(x).shape)
    if len(sx) < 1 or sx[0] < 1:
        raise ValueError('x must be (nrec, ...) with at least one record, got shape %s' % (sx,))
    S = sx[1:]
    n = int(np.prod(S, dtype=np.int64))
    if n < 1:
        raise ValueError('x has no cells: shape %s' % (sx,))
    mask = np.ascontiguousarray(mask_values, dtype=np.float64).reshape(-1)
    if mask.size > 2:
        raise ValueError('at most two mask values (_FillValue, missing_value), got %d' % mask.size)
    if base is not None:
        sb = tuple(raw(base).shape)
        lead = len(sb) - len(S)
        if lead < 0 or sb[lead:] != S or any(k != 1 for k in sb[:lead]):
            raise ValueError('base of shape %s does not take the mean of x %s: it must be %s, or that behind axes of length 1'
                             % (sb, sx, S))
        if out is not None and not (isinstance(out, DeviceArray) and isinstance(raw(base), DeviceArray)
                                    and out.shape == sb and out.dtype == raw(base).dtype):
            raise ValueError('out must be a DeviceArray of the shape and dtype of a DeviceArray base')
    elif out is not None or mask.size:
        raise ValueError('out and mask_values need a base')
    return sx[0], n, S, mask


def _time_mean_add(base, x, mask_values=(), out=None, want_mean=False):
    """One `pgw_time_mean_add` call -> (out, mean, n_masked, n_new_nan) as DeviceArrays / ints (out, mean: None when not
    asked for)."""
    nrec, n, S, mask = _mean_add_plan(base, x, mask_values, out)
    ctx = default_context()
    d_x = dev_own(ctx, x, (nrec, n))
    d_b = dev_own(ctx, base)
    if d_b is not None and out is None:
        out = ctx.empty(d_b.shape, d_b.dtype)
    d_m = ctx.empty(S, d_x.dtype) if (want_mean or d_b is None) else None
    n_masked, n_new_nan = C.c_longlong(0), C.c_longlong(0)
    ctx._check(ctx.lib.pgw_time_mean_add(ctx.handle, dtype_tag(d_x.dtype if d_b is None else d_b.dtype), dtype_tag(d_x.dtype),
                                         nrec, n, ptr(d_b), mask.size, mask.ctypes.data_as(_dp) if mask.size else None,
                                         d_x.ptr, ptr(out), ptr(d_m), C.byref(n_masked), C.byref(n_new_nan)))
    return out, d_m, n_masked.value, n_new_nan.value


def time_mean(x):
    """Mean over the leading axis of x (nrec, ...), NaN records left out: `delta_ts.mean(dim=['time'])` of the reference's
    postproc_cosmo/extpar_adapt.py:29, which xarray evaluates as `np.nanmean(values, axis=0)` - a sum in x's dtype in record
    order with NaN replaced by +0.0, divided by the count; NaN where every record is NaN.  The result has x's dtype and
    kind (ndarray, DeviceArray, or a labelled array without the leading dimension)."""
    mean = _time_mean_add(None, x)[1]
    if isinstance(x, DeviceArray):
        return mean
    host = mean.numpy()
    if is_labelled(x) and hasattr(x, 'like'):
        return x.like(host, tuple(x.dims)[1:])
    return host


def time_mean_add(base, x, mask_values=(), counts=False, out=None):
    """base + time_mean(x) where base is not a mask value: `ext_file['T_CL'][:] += delta_ts_clim.values.squeeze()` of the
    reference's postproc_cosmo/extpar_adapt.py:32 (numpy's in-place add on netCDF4's masked array).  x (nrec,) + S; base S,
    or S behind leading axes of length 1; the result has base's shape, dtype and kind.  The addition runs in the promoted
    type of the two and is rounded once to base's dtype.  mask_values: up to two values (`_FillValue`, `missing_value`);
    cells of base equal to one of them (NaN cells for a NaN value) keep their bits.  counts=True: (out, dict(n_masked,
    n_new_nan, mean)) - the masked cells, the unmasked ones that were not NaN and are now, and the mean that was added
    (shape S, x's dtype, the kind of out), all from the one launch.  out: for a DeviceArray base, the DeviceArray that
    takes the result (base itself: in place).  ValueError for shapes that do not fit, before the device is touched."""
    res, mean, n_masked, n_new_nan = _time_mean_add(base, x, mask_values, out, want_mean=counts)
    res = out_like(res, base)
    if not counts:
        return res
    return res, dict(n_masked=n_masked, n_new_nan=n_new_nan, mean=mean if isinstance(res, DeviceArray) else mean.numpy())


# ------------------------------------------------------------------------------- regridding
def regrid_tables(src_lat, src_lon, targ_lat, targ_lon):
    """Index/weight tables for the separable lat-then-lon linear interpolation of
    regrid_lat_lon's xarray branch (reference functions.py:774-789, 817-893), including its
    pole rows, periodic +-360 extension and scipy-interp1d index rule (searchsorted-left,
    clip to [1, n-1]).  Raises the reference's ValueErrors for uncovered targets."""
    src_lat = np.asarray(src_lat, dtype=np.float64)
    src_lon = np.asarray(src_lon, dtype=np.float64)
    targ_lat = np.asarray(targ_lat, dtype=np.float64)
    targ_lon = np.asarray(targ_lon, dtype=np.float64)
    nlat_s, nlon_s = len(src_lat), len(src_lon)
    dlon = np.median(np.diff(src_lon))                          # :778
    dlat = np.median(np.diff(src_lat))                          # :779 (before the flip)
    periodic = (dlon + np.max(src_lon) - np.min(src_lon)) >= 359.9     # :780-789
    rows = np.arange(nlat_s)
    lat = src_lat
    if lat[0] > lat[-1]:                                        # :822-829
        lat = lat[::-1]
        rows = rows[::-1]
    south_row = north_row = -1
    if np.max(targ_lat) + dlat > 89.9:                          # :833-837
        north_row = int(rows[-1])
        lat = np.concatenate([lat, [90.0]])
        rows = np.concatenate([rows, [nlat_s]])
    if np.min(targ_lat) - dlat < -89.9:                         # :838-842
        south_row = int(rows[0])
        lat = np.concatenate([[-90.0], lat])
        rows = np.concatenate([[-1], rows])
    if (np.max(targ_lat) > np.max(lat)) | (np.min(targ_lat) < np.min(lat)):      # :845-856
        raise ValueError('ERA5 dataset extends further North or South than GCM dataset!. Perhaps consider '
                         'using ERA5 on a subdomain only if global coverage is not required?')
    order = np.argsort(lat, kind='stable')                      # xarray sorts before interp
    lat, rows = lat[order], rows[order]
    idx = np.searchsorted(lat, targ_lat).clip(1, len(lat) - 1)
    lat_lo, lat_hi = rows[idx - 1].astype(np.int32), rows[idx].astype(np.int32)
    lat_dx = targ_lat - lat[idx - 1]
    lat_Dx = lat[idx] - lat[idx - 1]
    lat_oob = ((targ_lat < lat[0]) | (targ_lat > lat[-1])).astype(np.int32)

    lon = src_lon
    cols = np.arange(nlon_s)
    if periodic:                                                # :866-874
        if np.max(targ_lon) > np.max(lon):
            lon = np.concatenate([lon, src_lon + 360])
            cols = np.concatenate([cols, np.arange(nlon_s)])
        if np.min(targ_lon) < np.min(lon):
            lon = np.concatenate([lon - 360, lon])
            cols = np.concatenate([cols, cols])
    if (np.max(targ_lon) > np.max(lon)) | (np.min(targ_lon) < np.min(lon)):      # :877-888
        raise ValueError('ERA5 dataset extends further East or West than GCM dataset!. Perhaps consider '
                         'using ERA5 on a subdomain only if global coverage is not required?')
    order = np.argsort(lon, kind='stable')
    lon, cols = lon[order], cols[order]
    idx = np.searchsorted(lon, targ_lon).clip(1, len(lon) - 1)
    lon_lo, lon_hi = cols[idx - 1].astype(np.int32), cols[idx].astype(np.int32)
    lon_dx = targ_lon - lon[idx - 1]
    lon_Dx = lon[idx] - lon[idx - 1]
    lon_oob = ((targ_lon < lon[0]) | (targ_lon > lon[-1])).astype(np.int32)
    return dict(lat_lo=lat_lo, lat_hi=lat_hi, lat_dx=lat_dx, lat_Dx=lat_Dx, lat_oob=lat_oob,
                lon_lo=lon_lo, lon_hi=lon_hi, lon_dx=lon_dx, lon_Dx=lon_Dx, lon_oob=lon_oob,
                south_row=south_row, north_row=north_row, periodic=bool(periodic))


def _regrid(function, field, src_lat, src_lon, targ_lat, targ_lon, points):
    """regrid_field (`points` False: the targets are the mesh of two axes) and regrid_points (True: lat / lon of one common
    shape): the tables of the flattened targets, then the field through pgw_regrid_bilinear / pgw_regrid_points."""
    ctx = default_context()
    tb = regrid_tables(src_lat, src_lon, targ_lat.ravel(), targ_lon.ravel())      # the extent errors, before any launch
    shp = raw(field).shape
    ops = OperandPlan(ctx, function, field=field)
    if len(shp) < 2 or shp[-2] != len(src_lat) or shp[-1] != len(src_lon):
        raise ValueError('field shape does not match the source coordinates')
    nfield = int(np.prod(shp[:-2], dtype=np.int64)) if len(shp) > 2 else 1
    c = {k: np.ascontiguousarray(v) for k, v in tb.items() if isinstance(v, np.ndarray)}
    if points:
        c['oob'] = np.ascontiguousarray(c['lat_oob'] | c['lon_oob'], dtype=np.int32)
        entry, targ_shape, targ_n = ctx.lib.pgw_regrid_points, targ_lat.shape, (targ_lat.size,)
        names = 'lat_lo lat_hi lat_dx lat_Dx lon_lo lon_hi lon_dx lon_Dx oob'
    else:
        entry, targ_shape, targ_n = ctx.lib.pgw_regrid_bilinear, (len(targ_lat), len(targ_lon)), (len(targ_lat), len(targ_lon))
        names = 'lat_lo lat_hi lat_dx lat_Dx lat_oob lon_lo lon_hi lon_dx lon_Dx lon_oob'
    d_src = ops.dev('field')
    out = ctx.empty(tuple(shp[:-2]) + targ_shape, ops.result)
    tabs = [c[k].ctypes.data_as(_ip if c[k].dtype == np.int32 else _dp) for k in names.split()]
    ctx._check(entry(ctx.handle, ops.tag('field'), nfield, shp[-2], shp[-1], *targ_n, d_src.ptr, *tabs,
                     tb['south_row'], tb['north_row'], out.ptr))
    return out_like(out, field)


def regrid_field(field, src_lat, src_lon, targ_lat, targ_lon):
    """Bilinear (lat, then lon) regridding of field (..., nlat_s, nlon_s) on the GPU."""
    return _regrid('regrid_field', field, src_lat, src_lon, np.asarray(targ_lat, dtype=np.float64),
                   np.asarray(targ_lon, dtype=np.float64), points=False)


class RegridPlan:
    """`regrid_field` for many calls on one (source grid, target mesh) pair: the tables of `regrid_tables` - the reference's
    extent errors are raised here, before anything is launched - uploaded once into device memory the plan owns
    (pgw_regrid_plan_create), and `apply` launches on the context's stream without allocating or synchronising
    (pgw_regrid_plan_apply).  Source and output are DeviceArrays and may differ in dtype: the output holds
    `regrid_field(src).astype(out.dtype)`, bit for bit - what a regridded file holds after the host's astype."""

    def __init__(self, src_lat, src_lon, targ_lat, targ_lon, max_nfield, ctx=None):
        self.ctx = ctx or default_context()
        targ_lat, targ_lon = np.asarray(targ_lat, dtype=np.float64), np.asarray(targ_lon, dtype=np.float64)
        if targ_lat.ndim != 1 or targ_lon.ndim != 1:
            raise ValueError('a regrid plan takes the two 1-D axes of a target mesh; got lat %s and lon %s'
                             % (targ_lat.shape, targ_lon.shape))
        tb = regrid_tables(src_lat, src_lon, targ_lat, targ_lon)
        self.src_shape, self.targ_shape = (len(src_lat), len(src_lon)), (len(targ_lat), len(targ_lon))
        self.max_nfield = int(max_nfield)
        c = {k: np.ascontiguousarray(v) for k, v in tb.items() if isinstance(v, np.ndarray)}
        names = 'lat_lo lat_hi lat_dx lat_Dx lat_oob lon_lo lon_hi lon_dx lon_Dx lon_oob'
        tabs = [c[k].ctypes.data_as(_ip if c[k].dtype == np.int32 else _dp) for k in names.split()]
        handle = C.c_void_p()
        self.ctx._check(self.ctx.lib.pgw_regrid_plan_create(self.ctx.handle, *self.src_shape, *self.targ_shape, *tabs,
                                                            tb['south_row'], tb['north_row'], self.max_nfield, C.byref(handle)))
        self.handle = handle.value

    def apply(self, src, out):
        """src (..., nlat_s, nlon_s) -> out (..., nlat_t, nlon_t), DeviceArrays with the same leading shape."""
        if self.handle is None:
            raise ValueError('the regrid plan has been freed')
        if (len(src.shape) < 2 or tuple(src.shape[-2:]) != self.src_shape or tuple(out.shape[-2:]) != self.targ_shape
                or tuple(src.shape[:-2]) != tuple(out.shape[:-2])):
            raise ValueError('regrid plan %s -> %s: source %s and output %s do not fit' % (self.src_shape, self.targ_shape,
                                                                                         src.shape, out.shape))
        nfield = int(np.prod(src.shape[:-2], dtype=np.int64))
        self.ctx._check(self.ctx.lib.pgw_regrid_plan_apply(self.ctx.handle, self.handle, dtype_tag(src.dtype), dtype_tag(out.dtype),
                                                           nfield, src.ptr, out.ptr))
        return out

    def free(self):
        if self.handle is not None and self.ctx.handle:
            self.ctx.lib.pgw_regrid_plan_destroy(self.ctx.handle, self.handle)
        self.handle = None

    def __del__(self):
        try:
            self.free()
        except Exception:                                       # noqa: BLE001 - interpreter shutdown
            pass


def regrid_points(field, src_lat, src_lon, targ_lat, targ_lon):
    """Bilinear (lat, then lon) regridding of field (..., nlat_s, nlon_s) onto point-wise targets on the GPU: `targ_lat` and
    `targ_lon` have one common shape of any rank >= 1 (2-D coordinates of a rotated-pole grid, a list of cells), target g
    lies at (targ_lat[g], targ_lon[g]) - what xarray's `.interp({lat: targ_lat}).interp({lon: targ_lon})` computes for
    coordinates over shared dimensions (reference functions.py:812-893).  Degrees.  Returns (...,) + the targets' shape;
    dtype and array kind as `regrid_field`, whose bits a mesh handed over as points reproduces."""
    targ_lat, targ_lon = np.asarray(targ_lat, dtype=np.float64), np.asarray(targ_lon, dtype=np.float64)
    if targ_lat.ndim < 1 or targ_lat.shape != targ_lon.shape:
        raise ValueError('point-wise targets need lat and lon of one common shape (rank >= 1); got %s and %s'
                         % (targ_lat.shape, targ_lon.shape))
    return _regrid('regrid_points', field, src_lat, src_lon, targ_lat, targ_lon, points=True)


# ------------------------------------------------------------------------------- winds on a rotated-pole target grid
# Not in the reference (its targets are lat-lon meshes, whose winds are geographic): a file on a `rotated_latitude_longitude`
# mapping stores GRID-RELATIVE components, U along increasing rlon and V along increasing rlat (include/pgw_hip.h).
def _same_shape(what, **xs):
    shapes = {k: tuple(raw(x).shape) for k, x in xs.items()}
    first = next(iter(shapes.values()))
    if len(first) < 1 or any(s != first for s in shapes.values()):
        raise ValueError('%s need one common shape (rank >= 1); got %s' % (what, ', '.join('%s %s' % kv for kv in shapes.items())))
    return first


def wind_rotation(lat, lon, pole_lat, pole_lon):
    """(cos, sin) of the angle between geographic east and grid east at the points (lat, lon) of a rotated grid whose north pole
    lies at geographic (pole_lat, pole_lon) - CF `grid_north_pole_latitude` / `grid_north_pole_longitude`; degrees
    (pgw_wind_rotation).  float64, of the coordinates' common shape (rank >= 1): DeviceArrays when both coordinates are,
    ndarrays otherwise.  (1, 0) at a pole of the rotated grid, NaN for a NaN coordinate."""
    shape = _same_shape('lat and lon', lat=lat, lon=lon)
    ctx = default_context()
    d_lat, d_lon = dev(ctx, lat, F64), dev(ctx, lon, F64)
    c, s = ctx.empty(shape, F64), ctx.empty(shape, F64)
    ctx._check(ctx.lib.pgw_wind_rotation(ctx.handle, c.size, d_lat.ptr, d_lon.ptr, float(pole_lat), float(pole_lon), c.ptr, s.ptr))
    if isinstance(lat, DeviceArray) and isinstance(lon, DeviceArray):
        return c, s
    return c.numpy(), s.numpy()


def _wind_pair(ua, va, cos, sin, trailing=None):
    """Shapes and the dtype of a (ua, va, cos, sin) call, checked before the device is touched: ua and va of one shape with
    `trailing` horizontal dimensions (default: those of cos / sin) -> (shape, number of planes, dtype - float32 only when both
    are -, shape of cos / sin)."""
    shape = _same_shape('ua and va', ua=ua, va=va)
    cs = _same_shape('cos and sin', cos=cos, sin=sin)
    trailing = len(cs) if trailing is None else trailing
    if len(shape) < trailing:
        raise ValueError('ua and va of shape %s have fewer than %d horizontal dimensions' % (shape, trailing))
    if 0 in shape or 0 in cs:
        raise ValueError('ua and va of shape %s, cos and sin of shape %s: an empty array' % (shape, cs))
    return shape, int(np.prod(shape[:len(shape) - trailing], dtype=np.int64)), common_dtype(ua, va), cs


def rotate_wind(ua, va, cos, sin, inverse=False):
    """Geographic (ua, va) -> grid-relative (u, v) = (ua cos - va sin, ua sin + va cos), or back with inverse=True
    (pgw_rotate_pair).  cos / sin as `wind_rotation` returns them; the trailing dimensions of ua and va are their shape.
    Computed in float64 and rounded once to the common dtype of ua and va - float32 only when both are; array kinds as
    everywhere (u like ua, v like va).  settings.function_dtype_flow has no say: there is no reference function to follow."""
    shape, nfield, dtype, cs = _wind_pair(ua, va, cos, sin)
    if shape[len(shape) - len(cs):] != cs:
        raise ValueError('ua and va of shape %s do not end in the shape %s of cos and sin' % (shape, cs))
    ctx = default_context()
    n = int(np.prod(cs, dtype=np.int64))
    d_u, d_v, d_c, d_s = dev(ctx, ua, dtype), dev(ctx, va, dtype), dev(ctx, cos, F64), dev(ctx, sin, F64)
    u, v = ctx.empty(shape, dtype), ctx.empty(shape, dtype)
    ctx._check(ctx.lib.pgw_rotate_pair(ctx.handle, dtype_tag(dtype), nfield, n, d_u.ptr, d_v.ptr, d_c.ptr, d_s.ptr, int(bool(inverse)),
                                       u.ptr, v.ptr))
    return out_like(u, ua), out_like(v, va)


def regrid_points_wind(ua, va, src_lat, src_lon, targ_lat, targ_lon, cos, sin):
    """`regrid_points` on ua and va (..., nlat_s, nlon_s) together and `rotate_wind` by the targets' cos / sin (their shape is
    the targets') in one launch (pgw_regrid_points_wind): (u, v) hold the bits of the three calls - each regridded value is
    rounded to the dtype before it is rotated.  The extent errors of `regrid_tables` are raised before any launch."""
    targ_lat, targ_lon = np.asarray(targ_lat, dtype=np.float64), np.asarray(targ_lon, dtype=np.float64)
    if targ_lat.ndim < 1 or targ_lat.shape != targ_lon.shape:
        raise ValueError('point-wise targets need lat and lon of one common shape (rank >= 1); got %s and %s'
                         % (targ_lat.shape, targ_lon.shape))
    shape, nfield, dtype, cs = _wind_pair(ua, va, cos, sin, 2)
    if cs != targ_lat.shape:
        raise ValueError('cos and sin of shape %s do not lie over the targets of shape %s' % (cs, targ_lat.shape))
    if shape[-2:] != (len(src_lat), len(src_lon)):
        raise ValueError('field shape does not match the source coordinates')
    ctx = default_context()
    tb = regrid_tables(src_lat, src_lon, targ_lat.ravel(), targ_lon.ravel())      # the extent errors, before any launch
    c = {k: np.ascontiguousarray(v) for k, v in tb.items() if isinstance(v, np.ndarray)}
    c['oob'] = np.ascontiguousarray(c['lat_oob'] | c['lon_oob'], dtype=np.int32)
    tabs = [c[k].ctypes.data_as(_ip if c[k].dtype == np.int32 else _dp)
            for k in 'lat_lo lat_hi lat_dx lat_Dx lon_lo lon_hi lon_dx lon_Dx oob'.split()]
    d_u, d_v, d_c, d_s = dev(ctx, ua, dtype), dev(ctx, va, dtype), dev(ctx, cos, F64), dev(ctx, sin, F64)
    u, v = (ctx.empty(shape[:-2] + targ_lat.shape, dtype) for _ in range(2))
    ctx._check(ctx.lib.pgw_regrid_points_wind(ctx.handle, dtype_tag(dtype), nfield, shape[-2], shape[-1], targ_lat.size, d_u.ptr,
                                              d_v.ptr, *tabs, tb['south_row'], tb['north_row'], d_c.ptr, d_s.ptr, u.ptr, v.ptr))
    return out_like(u, ua), out_like(v, va)


class PointsPlan:
    """`regrid_points` / `regrid_points_wind` for many calls on one (source grid, target list) pair, beside RegridPlan: targets
    of one common shape of rank >= 1, target g at (targ_lat[g], targ_lon[g]).  The tables of `regrid_tables` - the reference's
    extent errors are raised here, before anything is launched - and, with `pole` = (lat, lon) of the rotated grid's north
    pole, the cos / sin of `wind_rotation` are uploaded once into device memory the plan owns (pgw_points_plan_create); `apply`
    and `apply_wind` launch on the context's stream without allocating or synchronising.  Sources and outputs are DeviceArrays
    and may differ in dtype: the outputs hold `regrid_points(src).astype(out.dtype)` / `regrid_points_wind(...)` cast
    likewise, bit for bit - what a file regridded (and rotated) by step_02 holds after the host's astype."""

    def __init__(self, src_lat, src_lon, targ_lat, targ_lon, max_nfield, pole=None, ctx=None):
        self.ctx = ctx or default_context()
        targ_lat, targ_lon = np.asarray(targ_lat, dtype=np.float64), np.asarray(targ_lon, dtype=np.float64)
        if targ_lat.ndim < 1 or targ_lat.shape != targ_lon.shape:
            raise ValueError('point-wise targets need lat and lon of one common shape (rank >= 1); got %s and %s'
                             % (targ_lat.shape, targ_lon.shape))
        tb = regrid_tables(src_lat, src_lon, targ_lat.ravel(), targ_lon.ravel())
        self.src_shape, self.targ_shape = (len(src_lat), len(src_lon)), tuple(targ_lat.shape)
        self.max_nfield = int(max_nfield)
        self.pole = None if pole is None else (float(pole[0]), float(pole[1]))
        c = {k: np.ascontiguousarray(v) for k, v in tb.items() if isinstance(v, np.ndarray)}
        c['oob'] = np.ascontiguousarray(c['lat_oob'] | c['lon_oob'], dtype=np.int32)
        tabs = [c[k].ctypes.data_as(_ip if c[k].dtype == np.int32 else _dp)
                for k in 'lat_lo lat_hi lat_dx lat_Dx lon_lo lon_hi lon_dx lon_Dx oob'.split()]
        cs = (None, None)
        if self.pole is not None:
            d_lat, d_lon = (self.ctx.to_device(np.ascontiguousarray(x)) for x in (targ_lat, targ_lon))
            cs = (self.ctx.empty(self.targ_shape, F64), self.ctx.empty(self.targ_shape, F64))
            self.ctx._check(self.ctx.lib.pgw_wind_rotation(self.ctx.handle, targ_lat.size, d_lat.ptr, d_lon.ptr, *self.pole,
                                                           cs[0].ptr, cs[1].ptr))
        handle = C.c_void_p()
        self.ctx._check(self.ctx.lib.pgw_points_plan_create(self.ctx.handle, *self.src_shape, targ_lat.size, *tabs, tb['south_row'],
                                                            tb['north_row'], self.max_nfield, ptr(cs[0]), ptr(cs[1]),
                                                            C.byref(handle)))
        self.handle = handle.value
        if self.pole is not None:                               # the plan holds its own copy (create has synchronised)
            for x in (d_lat, d_lon) + cs:
                x.free()

    def _nfield(self, srcs, outs):
        if self.handle is None:
            raise ValueError('the points plan has been freed')
        nt = len(self.targ_shape)
        lead = tuple(srcs[0].shape[:-2])
        if (any(len(s.shape) < 2 or tuple(s.shape[-2:]) != self.src_shape or tuple(s.shape[:-2]) != lead for s in srcs)
                or any(len(o.shape) < nt or tuple(o.shape[len(o.shape) - nt:]) != self.targ_shape
                       or tuple(o.shape[:len(o.shape) - nt]) != lead for o in outs)):
            raise ValueError('points plan %s -> %s: sources %s and outputs %s do not fit'
                             % (self.src_shape, self.targ_shape, [tuple(s.shape) for s in srcs], [tuple(o.shape) for o in outs]))
        if len({s.dtype for s in srcs}) != 1 or len({o.dtype for o in outs}) != 1:
            raise ValueError('points plan: the sources must share one dtype and the outputs one')
        return int(np.prod(lead, dtype=np.int64))

    def apply(self, src, out):
        """src (..., nlat_s, nlon_s) -> out (...,) + the targets' shape, DeviceArrays with the same leading shape."""
        nfield = self._nfield((src,), (out,))
        self.ctx._check(self.ctx.lib.pgw_points_plan_apply(self.ctx.handle, self.handle, dtype_tag(src.dtype), dtype_tag(out.dtype),
                                                           nfield, src.ptr, out.ptr))
        return out

    def apply_wind(self, src_u, src_v, out_u, out_v):
        """ua, va (..., nlat_s, nlon_s) -> grid-relative u, v (...,) + the targets' shape; the plan needs a `pole`."""
        nfield = self._nfield((src_u, src_v), (out_u, out_v))
        if self.pole is None:
            raise ValueError('the points plan was made without a pole and cannot rotate')
        self.ctx._check(self.ctx.lib.pgw_points_plan_apply_wind(self.ctx.handle, self.handle, dtype_tag(src_u.dtype),
                                                                dtype_tag(out_u.dtype), nfield, src_u.ptr, src_v.ptr, out_u.ptr,
                                                                out_v.ptr))
        return out_u, out_v

    def free(self):
        if self.handle is not None and self.ctx.handle:
            self.ctx.lib.pgw_points_plan_destroy(self.ctx.handle, self.handle)
        self.handle = None

    def __del__(self):
        try:
            self.free()
        except Exception:                                       # noqa: BLE001 - interpreter shutdown
            pass


# ------------------------------------------------------------------------------- regridding, 2-D source coordinates
def unit_vectors(lat_deg, lon_deg):
    """(..., 3) unit vectors (cos lat cos lon, cos lat sin lon, sin lat) of points in degrees, float64: the only
    trigonometry of the curvilinear regridding; the kernels work on these."""
    la = np.deg2rad(np.asarray(lat_deg, dtype=np.float64))
    lo = np.deg2rad(np.asarray(lon_deg, dtype=np.float64))
    return np.stack([np.cos(la) * np.cos(lo), np.cos(la) * np.sin(lo), np.sin(la)], axis=-1)


def pole_vector(row):
    """normalise(sum_i row[i]) of an edge row of node vectors (nx, 3), summed in index order."""
    s = np.add.accumulate(np.asarray(row, dtype=np.float64), axis=0)[-1]
    return s / np.sqrt((s[0] * s[0] + s[1] * s[1]) + s[2] * s[2])


def periodic_lon_rule(lon):
    """`periodic_lon` of regrid_lat_lon (reference functions.py:778-789) for 1-D or 2-D longitudes: np.diff along the
    last axis, its median, global max / min."""
    lon = np.asarray(lon, dtype=np.float64)
    return bool((np.median(np.diff(lon)) + np.max(lon) - np.min(lon)) >= 359.9)


def curvilinear_cells(X, periodic):
    """Corners of every cell of the node grid X (ny, nx, 3) in cell-number order: quads j * ncx + i (A, B, C, D), then -
    periodic only - the cap triangles of row 0 and of row ny - 1 as (pole, X_i, X_i+1, X_i+1).  Returns (ncell, 4, 3)."""
    ny, nx = X.shape[:2]
    ncx = nx if periodic else nx - 1
    ip = (np.arange(ncx) + 1) % nx
    i0 = np.arange(ncx)
    quads = np.stack([X[:-1][:, i0], X[:-1][:, ip], X[1:][:, ip], X[1:][:, i0]], axis=2).reshape(-1, 4, 3)
    if not periodic:
        return quads
    tris = []
    for je in (0, ny - 1):
        n = np.broadcast_to(pole_vector(X[je]), (nx, 3))
        tris.append(np.stack([n, X[je][i0], X[je][ip], X[je][ip]], axis=1))
    return np.concatenate([quads] + tris, axis=0)


def curvilinear_buckets(X, periodic, nb=None):
    """The candidate lists of k_cell_locate: a uniform nb^3 bucket grid over [-1, 1]^3 (only the shell around the sphere is
    occupied), every cell listed - ascending - in each bucket its bounding box touches.  The box is enlarged because a target
    P of the cell is the OUTWARD projection of a patch point p (a convex combination of the corners, so inside their box and
    inside the sphere): |P - p| = 1 - |p|, and with d the largest corner distance |p|^2 = sum w_k w_l X_k.X_l >=
    1 - d^2 / 2, so the radial bulge is at most 1 - sqrt(1 - d^2 / 2); plus 1e-8 for the acceptance tolerance (1e-10 in
    s, t moves p by less than 1e-9) and rounding.  A cell with a NaN corner accepts nothing and is listed nowhere.
    Returns (nb, bucket_start (nb^3 + 1) int32, bucket_cells int32)."""
    cells = curvilinear_cells(np.asarray(X, dtype=np.float64), periodic)
    ncell = len(cells)
    if nb is None:
        nb = int(min(max(int(np.sqrt(ncell / 2.0)), 1), 128))
    ok = np.isfinite(cells).all(axis=(1, 2))
    cid = np.nonzero(ok)[0]
    c = cells[ok]
    d2 = np.zeros(len(c))
    for a in range(4):
        for b in range(a + 1, 4):
            d2 = np.maximum(d2, ((c[:, a] - c[:, b]) ** 2).sum(axis=1))
    pad = (1.0 - np.sqrt(np.maximum(0.0, 1.0 - 0.5 * d2))) * (1.0 + 1e-6) + 1e-8

    def coord(x):
        return np.clip(((x + 1.0) * 0.5 * nb).astype(np.int64), 0, nb - 1)      # bucket_coord of pgw_kernels.h
    lo = coord(np.maximum(c.min(axis=1) - pad[:, None], -1.0))
    hi = coord(np.minimum(c.max(axis=1) + pad[:, None], 1.0))
    ext = hi - lo + 1
    cnt = ext.prod(axis=1)
    first = np.concatenate([[0], np.cumsum(cnt)])
    owner = np.repeat(np.arange(len(c)), cnt)
    k = np.arange(first[-1]) - first[owner]
    ez, ey = ext[owner, 2], ext[owner, 1]
    bz = lo[owner, 2] + k % ez
    by = lo[owner, 1] + (k // ez) % ey
    bx = lo[owner, 0] + k // (ez * ey)
    bucket = (bx * nb + by) * nb + bz
    order = np.lexsort((cid[owner], bucket))
    bucket_start = np.searchsorted(bucket[order], np.arange(nb ** 3 + 1)).astype(np.int32)
    return nb, bucket_start, np.ascontiguousarray(cid[owner][order].astype(np.int32))


class CurvilinearWeights:
    """Result of the locate phase: device-resident idx (ntarg, 4) int32 and w (ntarg, 4) float64, the unmapped count, and
    the shapes `regrid_curvilinear` needs."""

    def __init__(self, idx, w, n_unmapped, src_shape, targ_shape, periodic):
        self.idx, self.w, self.n_unmapped = idx, w, int(n_unmapped)
        self.src_shape, self.targ_shape, self.periodic = tuple(src_shape), tuple(targ_shape), bool(periodic)


def _mesh(lat, lon, what):
    lat, lon = np.asarray(lat, dtype=np.float64), np.asarray(lon, dtype=np.float64)
    if lat.ndim == 1 and lon.ndim == 1:
        return np.meshgrid(lat, lon, indexing='ij')
    if lat.ndim == 2 and lat.shape == lon.shape:
        return lat, lon
    raise ValueError('%s coordinates must be 1-D lat and lon or 2-D arrays of one shape' % what)


def locate_points(X, P, periodic, nb=None):
    """The locate phase on given vectors: nodes X (ny, nx, 3), targets P (ntarg, 3).  Returns CurvilinearWeights with a
    flat target shape."""
    ctx = default_context()
    X = np.ascontiguousarray(X, dtype=np.float64)
    P = np.ascontiguousarray(P, dtype=np.float64).reshape(-1, 3)
    if X.ndim != 3 or X.shape[2] != 3 or X.shape[0] < 2 or X.shape[1] < 2:
        raise ValueError('the source grid must be at least 2 x 2 nodes')
    if len(P) == 0:
        raise ValueError('no target points')
    ny, nx = X.shape[:2]
    nb, bstart, bcells = curvilinear_buckets(X, periodic, nb)
    nodes = X.reshape(-1, 3)
    if periodic:
        nodes = np.concatenate([nodes, pole_vector(X[0])[None], pole_vector(X[ny - 1])[None]], axis=0)
    f64 = np.dtype('float64')
    d_P, d_X = ctx.to_device(P, f64), ctx.to_device(np.ascontiguousarray(nodes), f64)
    d_bs = ctx.empty(bstart.shape, np.int32).copy_from(bstart)
    d_bc = ctx.empty((max(len(bcells), 1),), np.int32).copy_from(bcells if len(bcells) else np.zeros(1, np.int32))
    idx, w = ctx.empty((len(P), 4), np.int32), ctx.empty((len(P), 4), f64)
    n_un = C.c_longlong(0)
    ctx._check(ctx.lib.pgw_bilinear_locate(ctx.handle, len(P), d_P.ptr, ny, nx, 1 if periodic else 0, d_X.ptr, nb, d_bs.ptr,
                                           d_bc.ptr, idx.ptr, w.ptr, C.byref(n_un)))
    return CurvilinearWeights(idx, w, n_un.value, (ny, nx), (len(P),), periodic)


_WEIGHTS_CACHE = {}


def curvilinear_weights(src_lat, src_lon, targ_lat, targ_lon, periodic):
    """Locate phase of the bilinear regridding from a logically rectangular source grid with 1-D or 2-D coordinates onto
    target points with 1-D or 2-D coordinates (1-D pairs are meshed): what `xe.Regridder(ds_in, ds_era5, "bilinear",
    periodic=periodic)` computes (reference functions.py:799-800).  Cached per coordinate arrays, so the variables and files
    of one step_02 run locate once."""
    import hashlib
    from . import settings as S
    ctx = default_context()
    digest = hashlib.blake2b(digest_size=16)
    shapes = []
    for a in (src_lat, src_lon, targ_lat, targ_lon):          # the coordinates as given: nothing is meshed or copied on a hit
        a = np.ascontiguousarray(a, dtype=np.float64)
        shapes.append(a.shape)
        digest.update(a.data)
    key = (id(ctx), bool(periodic), tuple(shapes), digest.digest())
    hit = _WEIGHTS_CACHE.get(key)
    if hit is None:
        sla, slo = _mesh(src_lat, src_lon, 'source')
        tla, tlo = _mesh(targ_lat, targ_lon, 'target')
        hit = locate_points(unit_vectors(sla, slo), unit_vectors(tla, tlo).reshape(-1, 3), periodic)
        hit.targ_shape = tla.shape
        _WEIGHTS_CACHE.clear()                                 # one grid pair at a time: the tables of a big pair are ~50 MB
        _WEIGHTS_CACHE[key] = hit
        if S.i_debug >= 1:
            print('Regridding: %d of %d target points lie in no source cell (unmapped).'
                  % (hit.n_unmapped, int(np.prod(hit.targ_shape))))
    return hit


def regrid_curvilinear(field, weights):
    """Apply phase: field (..., ny, nx) -> (...,) + target shape on the GPU, dtype and array kind as `regrid_field`.
    Unmapped targets get 0.0, or NaN with settings.xesmf_unmapped_to_nan."""
    from . import settings as S
    ctx = default_context()
    shp = raw(field).shape
    if len(shp) < 2 or tuple(shp[-2:]) != weights.src_shape:
        raise ValueError('field shape does not match the source coordinates')
    ops = OperandPlan(ctx, 'regrid_curvilinear', field=field)
    nfield = int(np.prod(shp[:-2], dtype=np.int64)) if len(shp) > 2 else 1
    ntarg = int(np.prod(weights.targ_shape, dtype=np.int64))
    d_src = ops.dev('field')
    out = ctx.empty(tuple(shp[:-2]) + weights.targ_shape, ops.result)
    ctx._check(ctx.lib.pgw_regrid_sparse(ctx.handle, ops.tag('field'), nfield, shp[-2], shp[-1], ntarg, d_src.ptr,
                                         weights.idx.ptr, weights.w.ptr, 1 if S.xesmf_unmapped_to_nan else 0, out.ptr))
    return out_like(out, field)


def regrid_curvilinear_wind(ua, va, weights, src_cos=None, src_sin=None, targ_cos=None, targ_sin=None):
    """Apply phase for the winds of a rotated-pole source grid, in one launch (pgw_regrid_sparse_wind): ua, va (..., ny, nx)
    GRID-RELATIVE on the source grid where src_cos / src_sin - `wind_rotation` of the source's 2-D coordinates and the source
    grid's pole, of shape weights.src_shape - are given, are turned to geographic, regridded with `weights`, and - where
    targ_cos / targ_sin of shape weights.targ_shape are given - rotated onto the targets' grid.  (u, v) hold the bits of
        ug, vg = rotate_wind(ua, va, src_cos, src_sin, inverse=True)
        ur, vr = regrid_curvilinear(ug, weights), regrid_curvilinear(vg, weights)
        u,  v  = rotate_wind(ur, vr, targ_cos, targ_sin)
    with the first / last line left out for a pair that is None.  dtype: float32 only when ua and va both are; array kinds as
    everywhere (u like ua, v like va).  Unmapped targets as `regrid_curvilinear`."""
    from . import settings as S
    shape = _same_shape('ua and va', ua=ua, va=va)
    if len(shape) < 2 or tuple(shape[-2:]) != weights.src_shape:
        raise ValueError('ua and va of shape %s do not match the source coordinates %s' % (shape, weights.src_shape))
    if 0 in shape:
        raise ValueError('ua and va of shape %s: an empty array' % (shape,))
    for what, c, s, over in (('src', src_cos, src_sin, weights.src_shape), ('targ', targ_cos, targ_sin, weights.targ_shape)):
        if (c is None) != (s is None):
            raise ValueError('%s_cos and %s_sin: both or neither' % (what, what))
        if c is not None and _same_shape('%s_cos and %s_sin' % (what, what), cos=c, sin=s) != over:
            raise ValueError('%s_cos and %s_sin of shape %s do not lie over the %s grid of shape %s'
                             % (what, what, tuple(raw(c).shape), 'source' if what == 'src' else 'target', over))
    dtype = common_dtype(ua, va)
    ctx = default_context()
    nfield = int(np.prod(shape[:-2], dtype=np.int64))
    ntarg = int(np.prod(weights.targ_shape, dtype=np.int64))
    d_u, d_v = dev(ctx, ua, dtype), dev(ctx, va, dtype)
    d_cs = [None if x is None else dev(ctx, x, F64) for x in (src_cos, src_sin, targ_cos, targ_sin)]
    p = [None if x is None else x.ptr for x in d_cs]
    u, v = (ctx.empty(tuple(shape[:-2]) + weights.targ_shape, dtype) for _ in range(2))
    ctx._check(ctx.lib.pgw_regrid_sparse_wind(ctx.handle, dtype_tag(dtype), nfield, shape[-2], shape[-1], ntarg, d_u.ptr, d_v.ptr,
                                              p[0], p[1], weights.idx.ptr, weights.w.ptr, 1 if S.xesmf_unmapped_to_nan else 0,
                                              p[2], p[3], u.ptr, v.ptr))
    return out_like(u, ua), out_like(v, va)


# ------------------------------------------------------------------------------- delta files
_DATASET_CACHE = {}


def _open_cached(path):
    """Delta files are read once per process (the reference re-opens them per call,
    functions.py:203-204, i.e. ~14x per ERA5 file plus once per iteration)."""
    from . import ncio
    key = os.path.abspath(path)
    st = os.stat(key)
    hit = _DATASET_CACHE.get(key)
    if hit is None or hit[0] != (st.st_mtime_ns, st.st_size):
        _DATASET_CACHE[key] = ((st.st_mtime_ns, st.st_size), ncio.open_dataset(key))
    return _DATASET_CACHE[key][1]


def load_delta(delta_input_dir, var_name, era5_date_time, target_date_time=None,
               name_base=file_name_bases['SCEN-HIST']):
    """Load a climate delta and, if target_date_time is given, interpolate it linearly to that
    time of the year (periodic, Feb-29 dropped).  reference functions.py:195-303.
    Returns a labelled array (time, [plev,] lat, lon); time has length 1 when interpolated and is
    stamped with `era5_date_time` (:296)."""
    from . import ncio
    from .step_03_apply_to_era import delta_time_bracket
    ds = _open_cached(os.path.join(delta_input_dir, name_base.format(var_name)))
    fld = ds[var_name]
    times = np.asarray(ds[TIME_GCM].values)
    if fld.dims[0] != TIME_GCM:
        raise ValueError('first dimension of %s must be %s' % (var_name, TIME_GCM))
    ib, ia, x_hi, x_new, keep = delta_time_bracket(times, times[0] if target_date_time is None else target_date_time)
    if target_date_time is None:                                    # :298-301
        return ncio.Field(fld.values[keep], fld.dims, dict(fld.coords, **{TIME_GCM: times[keep]}), fld.attrs, var_name)
    vb = fld.values[keep[ib]]
    if x_hi == 0.0:                                                 # :282-283
        val = np.array(vb, copy=True)
    else:                                                           # :288-292 on the GPU
        val = time_lerp(vb, fld.values[keep[ia]], x_hi, x_new)
    t = np.asarray(getattr(era5_date_time, 'values', era5_date_time)).reshape(-1)[:1]
    coords = dict(fld.coords)
    coords[TIME_GCM] = t
    return ncio.Field(val[None], fld.dims, coords, fld.attrs, var_name)


def load_delta_interp(delta_input_dir, var_name, target_P, era5_date_time, target_date_time,
                      ignore_top_pressure_error=False):
    """load_delta + (for ta, hur) the surface delta and HIST surface pressure + vertical
    interpolation onto the model levels.  reference functions.py:306-340."""
    delta = load_delta(delta_input_dir, var_name, era5_date_time, target_date_time)
    if var_name in ['ta', 'hur']:
        delta_sfc = load_delta(delta_input_dir, var_name + 's', era5_date_time, target_date_time)
        ps_hist = load_delta(delta_input_dir, 'ps', era5_date_time, target_date_time,
                             name_base=file_name_bases['HIST'])
    else:
        delta_sfc = ps_hist = None
    return vert_interp_delta(delta, target_P, delta_sfc, ps_hist, ignore_top_pressure_error)


# ------------------------------------------------------------------------------- step_02
def _curvilinear_source(ds_gcm, ds_era5, var_name):
    """What the xESMF branch takes from its files before it regrids `var_name`: -> (weights, values (..., ny, nx) as the
    kernels take them).  ValueError when the variable does not end in the source grid's horizontal dimensions."""
    from . import settings as S
    src_lat, src_lon = np.asarray(ds_gcm[LAT_GCM].values), np.asarray(ds_gcm[LON_GCM].values)
    periodic_lon = periodic_lon_rule(src_lon)                   # :778-789
    if periodic_lon and S.i_debug >= 1:
        print('Regridding: Use periodic boundary conditions for GCM input data as it appears to be periodic in '
              'longitudinal direction.')
    hdims = tuple(ds_gcm[LAT_GCM].dims) if src_lat.ndim == 2 else (LAT_GCM, LON_GCM)
    f = ds_gcm[var_name]
    if tuple(f.dims[-2:]) != hdims:
        raise ValueError('%s has dimensions %s; its last two must be the horizontal dimensions %s of the source grid'
                         % (var_name, tuple(f.dims), hdims))
    targ_lat, targ_lon = (np.asarray(ds_era5[c].values, dtype=np.float64) for c in (LAT_ERA, LON_ERA))
    weights = curvilinear_weights(src_lat, src_lon, targ_lat, targ_lon, periodic_lon)          # xe.Regridder  :799-800
    vals = f.values                                            # float32 / float64 of either byte order keep their width
    vals = vals.astype(vals.dtype.newbyteorder('=') if vals.dtype.kind == 'f' and vals.dtype.itemsize in (4, 8) else np.float64,
                       copy=False)
    return weights, np.ascontiguousarray(vals)


def _regrid_lat_lon_curvilinear(ds_gcm, ds_era5, var_name, given=None):
    """The xESMF branch of regrid_lat_lon (reference functions.py:797-810) on the GPU.  given (not in the reference):
    (values, attributes) - the values of `var_name` on the target grid the caller has already (regrid_lat_lon_source_wind);
    the variable gets them and the attributes in place of its own, nothing else about the result differs."""
    from . import ncio
    f = ds_gcm[var_name]
    t_lat, t_lon = ds_era5[LAT_ERA], ds_era5[LON_ERA]
    targ_lat, targ_lon = np.asarray(t_lat.values, dtype=np.float64), np.asarray(t_lon.values, dtype=np.float64)
    if given is None:
        weights, vals = _curvilinear_source(ds_gcm, ds_era5, var_name)
        res = regrid_curvilinear(vals, weights)                                                # regridder(...)  :802
    else:
        res = given[0]
    lead = tuple(f.dims[:-2])
    out = ncio.Dataset(attrs=ds_gcm.attrs)                                                     # :810
    for d in lead:
        if d in ds_gcm:
            out[d] = ds_gcm[d]
    # 2-D target coordinates lie over their own dimensions; 1-D ones are the axes of a mesh here, whatever their dimensions
    tg = _Target(targ_lat, targ_lon, targ_lat.ndim == 2, t_lat.dims if targ_lat.ndim == 2 else (LAT_GCM, LON_GCM))
    tg.put_coords(out)
    tg.put_field(out, var_name, res, lead, {d: f.coords[d] for d in lead if d in f.coords})
    if 'height' in ds_gcm and 'height' not in out:
        out['height'] = ds_gcm['height']
    for name in [var_name, TIME_GCM, PLEV_GCM, LAT_GCM, LON_GCM, 'height']:                   # :805-808
        if name in ds_gcm and name in out:
            attrs = given[1] if given is not None and name == var_name else ds_gcm[name].attrs
            out[name] = ncio.Field(out[name].values, out[name].dims, out[name].coords, attrs, name)
    return out


def _target_layout(lat_dims, lat_shape, lon_dims, lon_shape):
    """How a target's lat / lon lie: (False, (lat, lon)) for two 1-D axes over dimensions of their own (a mesh),
    (True, their dimensions) for coordinates over the same dimensions (2-D coordinates of a rotated-pole grid, one `cell`
    dimension: point by point); any other combination is a ValueError.  The rule of regrid_lat_lon and of the ocean-grid
    branch of interp_wrapper."""
    lat_dims, lon_dims, lat_shape, lon_shape = tuple(lat_dims), tuple(lon_dims), tuple(lat_shape), tuple(lon_shape)
    if len(lat_shape) == 1 and len(lon_shape) == 1 and lat_dims != lon_dims:
        return False, (LAT_GCM, LON_GCM)
    if len(lat_shape) >= 1 and lat_dims == lon_dims and lat_shape == lon_shape:
        return True, lat_dims
    raise ValueError('target %s %s over %s and %s %s over %s are neither two 1-D axes of a mesh nor point-wise coordinates '
                     'over the same dimensions' % (LAT_ERA, lat_shape, lat_dims, LON_ERA, lon_shape, lon_dims))


class _Target:
    """A target grid of step_02: `lat` / `lon` [deg] as float64 arrays, `points` and `dims` as _target_layout names them,
    and how results are written onto it: lat / lon as 1-D axes that are their own coordinates (a mesh), or as variables
    over the target's dimensions (point-wise), a result over its leading dimensions + `dims` either way."""

    def __init__(self, lat, lon, points, dims):
        self.lat, self.lon = np.asarray(lat, dtype=np.float64), np.asarray(lon, dtype=np.float64)
        self.points, self.dims = bool(points), tuple(dims)

    @classmethod
    def of(cls, t_lat, t_lon, field_dims=()):
        """By the rule of _target_layout, from labelled lat / lon; a bare array is an axis of its own name when it is 1-D
        and `field_dims` (the dimensions of the field it is a coordinate of) have that name, else it lies over them."""
        def dims_of(c, name):
            if hasattr(c, 'dims'):
                return tuple(c.dims)
            return (name,) if np.ndim(c) == 1 and name in field_dims else tuple(field_dims)
        points, dims = _target_layout(dims_of(t_lat, LAT_ERA), np.shape(t_lat), dims_of(t_lon, LON_ERA), np.shape(t_lon))
        return cls(getattr(t_lat, 'values', t_lat), getattr(t_lon, 'values', t_lon), points, dims)

    def put_coords(self, ds, lat_attrs=None, lon_attrs=None):
        from . import ncio
        for name, x, attrs in ((LAT_GCM, self.lat, lat_attrs), (LON_GCM, self.lon, lon_attrs)):
            ds[name] = ncio.Field(x, self.dims, {}, attrs) if self.points else ncio.Field(x, (name,), {name: x}, attrs)

    def put_field(self, ds, name, values, lead, lead_coords, attrs=None):
        from . import ncio
        coords = dict(lead_coords) if self.points else dict(lead_coords, **{LAT_GCM: self.lat, LON_GCM: self.lon})
        ds[name] = ncio.Field(values, tuple(lead) + self.dims, coords, attrs)


def _horizontal_values(f):
    """A (..., lat, lon) variable of a GCM file as regrid_lat_lon hands it to the kernels: (leading dimensions, values with
    lat and lon last, float32 / float64 as they are and anything else as float64)."""
    lead = [d for d in f.dims if d not in (LAT_GCM, LON_GCM)]
    g = f.transpose(*(lead + [LAT_GCM, LON_GCM]))
    return lead, g.values if g.values.dtype in (np.float32, np.float64) else g.values.astype(np.float64)


def regrid_lat_lon(ds_gcm, ds_era5, var_name, method='bilinear', i_use_xesmf=0, given=None):
    """Bilinear regridding onto the ERA5 grid of `ds_era5` (reference functions.py:748-898).  i_use_xesmf = 0: the xarray
    branch, every lat/lon variable of `ds_gcm` (1-D source coordinates) through the separable kernel when the target's lat
    and lon are 1-D axes of their own (a mesh), through `regrid_points` when they lie over the same dimensions (2-D
    coordinates of a rotated-pole file, one `cell` dimension): the result then lies on the target's dimensions and lat / lon
    are written as variables over them, like the xESMF branch does; any other combination is a ValueError.  i_use_xesmf = 1: the xESMF
    branch (:797-810) for source grids with 2-D coordinates (rotated-pole, curvilinear; 1-D ones are meshed), `var_name`
    through the cell-locate and sparse-apply kernels.  Returns a new Dataset on the target grid.
    given (not in the reference; xarray branch): {name: (values, attributes)} - variables whose values on the target grid the
    caller has already (regrid_lat_lon_wind), laid out as this function would lay them out; they get the attributes on top of
    their own and nothing else about the result differs."""
    from . import ncio
    if i_use_xesmf:
        return _regrid_lat_lon_curvilinear(ds_gcm, ds_era5, var_name)
    src_lon = np.asarray(ds_gcm[LON_GCM].values, dtype=np.float64)
    src_lat = np.asarray(ds_gcm[LAT_GCM].values, dtype=np.float64)
    # 1-D lat over its own dimension and 1-D lon over its own: a mesh.  lat and lon over the same dimensions (2-D coordinates
    # of a rotated-pole grid, one `cell` dimension): xarray interpolates point by point.
    tg = _Target.of(ds_era5[LAT_ERA], ds_era5[LON_ERA])
    regrid = regrid_points if tg.points else regrid_field
    out = ncio.Dataset(attrs=ds_gcm.attrs)
    for name, f in ds_gcm.variables.items():
        if name in (LAT_GCM, LON_GCM):
            continue
        if LAT_GCM in f.dims and LON_GCM in f.dims:
            lead, vals = _horizontal_values(f)
            if given and name in given:
                res, attrs = given[name][0], dict(f.attrs, **given[name][1])
            else:
                res, attrs = regrid(vals, src_lat, src_lon, tg.lat, tg.lon), f.attrs
            tg.put_field(out, name, res, lead, {d: f.coords[d] for d in lead if d in f.coords}, attrs)
        elif LAT_GCM not in f.dims and LON_GCM not in f.dims:
            out[name] = f
    tg.put_coords(out, ds_gcm[LAT_GCM].attrs, ds_gcm[LON_GCM].attrs)      # point-wise: laid out like the xESMF branch's 2-D target
    return out


WIND_MARKER = dict(wind_components='grid_relative')      # on a ua / va variable whose components follow the target's rotated grid


def rotated_pole_of(ds, var_name, flag='--rotate_winds', file='target file'):
    """(grid_north_pole_latitude, grid_north_pole_longitude) of the rotated grid of a file: from the variable the
    `grid_mapping` attribute of `var_name` names; where the file has no such variable or attribute, from its only variable
    with grid_mapping_name = 'rotated_latitude_longitude'.  ValueError when there is none, more than one, or no pole on it;
    `flag` and `file` are the words its messages name the command-line flag and the file with."""
    rotated = [n for n, f in ds.variables.items() if f.attrs.get('grid_mapping_name') == 'rotated_latitude_longitude']
    named = ds[var_name].attrs.get('grid_mapping') if var_name is not None and var_name in ds else None
    if named is not None:
        if named not in rotated:
            raise ValueError("%s auto: the grid_mapping '%s' of %s is not a variable with grid_mapping_name = "
                             "'rotated_latitude_longitude': no rotated mapping found; give the pole as POLE_LAT,POLE_LON"
                             % (flag, named, var_name))
        rotated = [named]
    if not rotated:
        raise ValueError("%s auto: no rotated mapping found - the %s has no variable with "
                         "grid_mapping_name = 'rotated_latitude_longitude'; give the pole as POLE_LAT,POLE_LON" % (flag, file))
    if len(rotated) > 1:
        raise ValueError('%s auto: more than one rotated mapping in the %s (%s) and no grid_mapping '
                         'attribute on %s to choose one; give the pole as POLE_LAT,POLE_LON' % (flag, file, ', '.join(rotated), var_name))
    attrs = ds[rotated[0]].attrs
    try:
        return tuple(float(np.ravel(attrs[k])[0]) for k in ('grid_north_pole_latitude', 'grid_north_pole_longitude'))
    except KeyError as e:
        raise ValueError('%s auto: the rotated mapping %s of the %s has no %s' % (flag, rotated[0], file, e)) from None


def _curvilinear_dtype(f):
    """The dtype the xESMF branch regrids a variable in: float32 / float64 of either byte order, anything else as float64."""
    dt = np.asarray(f.values).dtype
    return dt.newbyteorder('=') if dt.kind == 'f' and dt.itemsize in (4, 8) else np.dtype(np.float64)


def check_wind_pair(ds_ua, ds_va, names=('ua', 'va'), flag='--rotate_winds', source_winds=False):
    """What regrid_lat_lon_wind needs of the two files of one period, checked before anything is computed or written:
    neither variable carries WIND_MARKER already (a second rotation), both lie on the same source grid, the same other
    dimensions (plev, number of records) and have the same dtype.  ValueError naming the cause, under the name `flag`.
    source_winds: the rule of regrid_lat_lon_source_wind - the caller states what the source's components follow, so a
    variable that carries the marker is accepted, and the dtype is the one the xESMF branch regrids in."""
    for ds, name in zip((ds_ua, ds_va), names):
        if not source_winds and ds[name].attrs.get('wind_components') == WIND_MARKER['wind_components']:
            raise ValueError("%s already carries wind_components = 'grid_relative': these files have been rotated onto a "
                             'rotated grid, rotating them again (double rotation) would be wrong' % name)
    fu, fv = ds_ua[names[0]], ds_va[names[1]]
    for c in (LAT_GCM, LON_GCM):
        if c not in ds_ua or c not in ds_va or not np.array_equal(np.asarray(ds_ua[c].values), np.asarray(ds_va[c].values)):
            raise ValueError(flag + ': %s and %s differ in their source grid (%s)' % (names[0], names[1], c))
    if tuple(fu.dims) != tuple(fv.dims):
        raise ValueError(flag + ': %s has dimensions %s, %s has %s' % (names[0], fu.dims, names[1], fv.dims))
    for d, nu, nv in zip(fu.dims, fu.shape, fv.shape):
        if d == PLEV_GCM and (nu != nv or not np.array_equal(np.asarray(ds_ua[d].values), np.asarray(ds_va[d].values))):
            raise ValueError(flag + ': %s and %s differ in plev' % names)
        if nu != nv:
            raise ValueError(flag + ': %s and %s differ in the number of records: %d and %d along %s'
                             % (names[0], names[1], nu, nv, d))
    kind = _curvilinear_dtype if source_winds else (lambda f: _horizontal_values(f)[1].dtype)
    if kind(fu) != kind(fv):
        raise ValueError(flag + ': %s and %s differ in dtype (%s, %s)' % (names[0], names[1], fu.dtype, fv.dtype))


def regrid_lat_lon_wind(ds_ua, ds_va, ds_era5, pole, names=('ua', 'va')):
    """`regrid_lat_lon` of a ua file and a va file onto a target with point-wise lat / lon on a rotated grid whose north
    pole lies at `pole` = (lat, lon), the two wind variables through `regrid_points_wind`: they come out GRID-RELATIVE, carry
    WIND_MARKER and the pole as attributes, and hold the bits of `rotate_wind` applied to what regrid_lat_lon writes.
    Everything else in the two datasets is regrid_lat_lon's.  Returns (ds_ua_out, ds_va_out)."""
    check_wind_pair(ds_ua, ds_va, names)
    tg = _Target.of(ds_era5[LAT_ERA], ds_era5[LON_ERA])
    if not tg.points:
        raise ValueError('the target has 1-D lat / lon axes: the winds of a lat-lon mesh are geographic already, there is '
                         'nothing to rotate')
    src_lat, src_lon = (np.asarray(ds_ua[c].values, dtype=np.float64) for c in (LAT_GCM, LON_GCM))
    cos, sin = wind_rotation(tg.lat, tg.lon, *pole)
    u, v = regrid_points_wind(_horizontal_values(ds_ua[names[0]])[1], _horizontal_values(ds_va[names[1]])[1], src_lat, src_lon,
                              tg.lat, tg.lon, cos, sin)
    attrs = dict(WIND_MARKER, grid_north_pole_latitude=np.float64(pole[0]), grid_north_pole_longitude=np.float64(pole[1]))
    return (regrid_lat_lon(ds_ua, ds_era5, names[0], given={names[0]: (u, attrs)}),
            regrid_lat_lon(ds_va, ds_era5, names[1], given={names[1]: (v, attrs)}))


WIND_POLE_ATTRS = ('grid_north_pole_latitude', 'grid_north_pole_longitude')


def regrid_lat_lon_source_wind(ds_ua, ds_va, ds_era5, source_pole, target_pole, names=('ua', 'va')):
    """The xESMF branch of `regrid_lat_lon` (i_use_xesmf = 1) of a ua file and a va file whose source grid is a rotated-pole
    grid with north pole at `source_pole` = (lat, lon) and whose winds are GRID-RELATIVE on it (None: they are geographic),
    onto the target of `ds_era5`; target_pole = (lat, lon): the target is a rotated grid (point-wise lat / lon) and the winds
    come out GRID-RELATIVE on it, with WIND_MARKER and the pole as `regrid_lat_lon_wind` writes them; None: they come out
    geographic and carry no marker, whatever the source variables carry.  The two wind variables go through
    `regrid_curvilinear_wind` (the bits of rotate_wind(inverse), regrid_curvilinear, rotate_wind); everything else in the two
    datasets is what regrid_lat_lon(i_use_xesmf=1) writes.  Returns (ds_ua_out, ds_va_out)."""
    check_wind_pair(ds_ua, ds_va, names, flag='--source_winds', source_winds=True)
    src_lat, src_lon = (np.asarray(ds_ua[c].values, dtype=np.float64) for c in (LAT_GCM, LON_GCM))
    if source_pole is not None and not (src_lat.ndim == 2 and src_lat.shape == src_lon.shape):
        raise ValueError('a source pole needs 2-D source coordinates: the winds of a source with 1-D lat / lon axes are '
                         'geographic already')
    if target_pole is not None and not _Target.of(ds_era5[LAT_ERA], ds_era5[LON_ERA]).points:
        raise ValueError('the target has 1-D lat / lon axes: the winds of a lat-lon mesh are geographic already, there is '
                         'nothing to rotate')
    weights, ua = _curvilinear_source(ds_ua, ds_era5, names[0])
    _, va = _curvilinear_source(ds_va, ds_era5, names[1])
    src_cs = wind_rotation(src_lat, src_lon, *source_pole) if source_pole is not None else (None, None)
    targ_cs = (None, None)
    if target_pole is not None:
        targ_cs = wind_rotation(*(np.asarray(ds_era5[c].values, dtype=np.float64) for c in (LAT_ERA, LON_ERA)), *target_pole)
    u, v = regrid_curvilinear_wind(ua, va, weights, *src_cs, *targ_cs)
    out = []
    for ds, name, values in ((ds_ua, names[0], u), (ds_va, names[1], v)):
        attrs = {k: a for k, a in ds[name].attrs.items() if k not in WIND_MARKER and k not in WIND_POLE_ATTRS}
        if target_pole is not None:
            attrs.update(WIND_MARKER, **dict(zip(WIND_POLE_ATTRS, (np.float64(target_pole[0]), np.float64(target_pole[1])))))
        elif not any(k in ds[name].attrs for k in WIND_MARKER):
            attrs = ds[name].attrs
        out.append(_regrid_lat_lon_curvilinear(ds, ds_era5, name, given=(values, attrs)))
    return tuple(out)


# ------------------------------------------------------------------------------- step_02 smoothing
def harmonic_tables(lt):
    """cos / sin(2 pi i / lt * t), t = 1..lt, i = 1..3, evaluated as the reference does (functions.py:716, 727)
    so the table entries are the same doubles: ([3][lt], [3][lt])."""
    import math
    tv = np.arange(1, lt + 1, 1)
    arg = [2. * math.pi * i / lt * tv for i in (1, 2, 3)]
    return (np.ascontiguousarray(np.stack([np.cos(a) for a in arg])),
            np.ascontiguousarray(np.stack([np.sin(a) for a in arg])))


def smooth_annual_cycle(diff):
    """Spectral smoothing of every column of a (time, [level,] y, x) array on the GPU (`pgw_harmonic_smooth`):
    the array form of filter_data (reference functions.py:603-669).  Returns the kind of `diff` (host array, labelled
    array or DeviceArray), same dtype."""
    ctx = default_context()
    r = raw(diff)
    if len(r.shape) not in (3, 4):
        raise ValueError('Wrong dimensions of input file should be 3 or 4-D')          # :648
    ops = OperandPlan(ctx, 'smooth_annual_cycle', diff=diff)
    lt = int(r.shape[0])
    inner = int(np.prod(r.shape[1:], dtype=np.int64))
    cos_t, sin_t = harmonic_tables(max(lt, 1))
    d_in = ops.dev('diff')
    d_out = ctx.empty(r.shape, ops.result)
    ctx._check(ctx.lib.pgw_harmonic_smooth(ctx.handle, ops.tag('diff'), lt, inner, cos_t.ctypes.data_as(_dp),
                                           sin_t.ctypes.data_as(_dp), d_in.ptr, d_out.ptr))
    return out_like(d_out, diff)


def harmonic_ac_analysis(ts):
    """Smoothed version of one series: mean + first three harmonics (reference functions.py:672-740); a series
    holding a NaN comes back all NaN in its own dtype, otherwise float64 like the reference.  Series shorter than 8
    steps: ValueError with the reference's text (the reference's `sys.exit` at :735 is a NameError, `sys` is not
    imported there)."""
    ts = np.asarray(ts)
    if ts.ndim != 1:
        raise ValueError('harmonic_ac_analysis expects a 1-D series')
    if np.isnan(ts).any():
        return np.full_like(ts, np.nan)
    out = smooth_annual_cycle(np.ascontiguousarray(ts, dtype=np.float64).reshape(-1, 1, 1))
    return out.reshape(-1)


def filter_data(annualcycleraw, variablename_to_smooth, outputpath):
    """File form (reference functions.py:603-669): read the variable, drop size-1 dimensions (`.squeeze()`), smooth
    every column along the first dimension, write the variable with its coordinates to `outputpath`."""
    from . import ncio
    ds = ncio.open_dataset(annualcycleraw)
    f = ds[variablename_to_smooth]
    keep = [i for i, n in enumerate(f.shape) if n != 1]
    vals = f.values.reshape([f.shape[i] for i in keep])
    dims = tuple(f.dims[i] for i in keep)
    print('Dimension that is assumed to be time dimension is called: ', dims[0] if dims else None)
    print('shape of data: ', vals.shape)
    if vals.dtype not in (np.float32, np.float64):
        vals = vals.astype(np.float64)
    res = smooth_annual_cycle(vals)
    print('Done with smoothing')
    out = ncio.Dataset(attrs={})
    for d in dims:
        if d in ds:
            out[d] = ds[d]
    out[variablename_to_smooth] = ncio.Field(res, dims, {d: f.coords[d] for d in dims if d in f.coords}, f.attrs)
    ncio.to_netcdf(out, outputpath)


# ------------------------------------------------------------------------------- step_02: ocean-grid deltas
def _fold_lon(lon):
    """functions.py:938-941 / 998-1001: longitudes above 180 move to the (-180, 180] range."""
    lon = np.array(lon, dtype=np.float64, copy=True)
    lon[lon > 180] -= 360
    return lon


def planar_metres(lat_deg, lon_deg):
    """The reference's point-cloud coordinates (functions.py:958-975, 1010-1023: three pyproj Geod.inv lengths per point) on
    the GPU (`pgw_planar_metres`): (lat_m, lon_m, lon_offset) in metres for latitudes / longitudes in degrees, longitudes
    already folded to (-180, 180].  The arithmetic is pgw4era5_amd/geodesy.py's (the host form, kept as the check)."""
    ctx = default_context()
    lat = np.ascontiguousarray(lat_deg, dtype=np.float64).reshape(-1)
    lon = np.ascontiguousarray(lon_deg, dtype=np.float64).reshape(-1)
    if lat.shape != lon.shape:
        raise ValueError('latitudes and longitudes must have the same number of points')
    n = len(lat)
    if n == 0:
        return np.zeros(0), np.zeros(0), np.zeros(0)
    f64 = np.dtype('float64')
    d_lat, d_lon = ctx.to_device(lat, f64), ctx.to_device(lon, f64)
    outs = [ctx.empty((n,), f64) for _ in range(3)]
    ctx._check(ctx.lib.pgw_planar_metres(ctx.handle, n, d_lat.ptr, d_lon.ptr, outs[0].ptr, outs[1].ptr, outs[2].ptr))
    return tuple(o.numpy() for o in outs)


def _ocean_source_values(gcm_lat, gcm_lon, fields):
    """The ocean grid's points as flat arrays: (lat (npoint), lon (npoint) folded, values (npoint, nfield))."""
    vals = np.stack([np.asarray(f, dtype=np.float64).reshape(-1) for f in fields], axis=1)       # (npoint, nfield)
    glat = np.asarray(gcm_lat, dtype=np.float64).reshape(-1)
    glon = _fold_lon(np.asarray(gcm_lon).reshape(-1))
    if not (glat.shape == glon.shape == vals.shape[:1]):
        raise ValueError('ocean-grid coordinates and values must have the same number of points')
    return glat, glon, vals


class _OceanCloud:
    """The source cloud of the ocean-grid interpolation on the device, as both gauss_interp_fields and gauss_interp_points
    hand it to their kernels: the points that are not NaN in every field, in planar metres, with the two shifted copies,
    sorted into square cells of one kernel radius (`cell_start`: first point of each cell)."""

    def __init__(self, ctx, gcm_lat, gcm_lon, fields, kernel_radius):
        glat, glon, vals = _ocean_source_values(gcm_lat, gcm_lon, fields)
        self.nf = nf = vals.shape[1]
        keep = ~np.isnan(vals).all(axis=1)                     # :944-948 (a point that is NaN in every field is in no cloud)
        glat, glon, vals = glat[keep], glon[keep], vals[keep]
        lat_m, lon_m, lon_off = planar_metres(glat, glon)                                       # :958-975
        # :977-991 the whole field once more to the left and to the right, shifted by twice the half-way-round length
        sx = np.tile(lat_m, 3)
        sy = np.concatenate([lon_m - 2 * lon_off, lon_m, lon_m + 2 * lon_off])
        sv = np.tile(vals, (3, 1))
        # uniform cells of one kernel radius over the source cloud
        self.h = h = float(kernel_radius)
        if len(sx):
            x0, y0 = float(sx.min()), float(sy.min())
            ncx, ncy = int((sx.max() - x0) // h) + 1, int((sy.max() - y0) // h) + 1
            cid = ((sx - x0) // h).astype(np.int64) * ncy + ((sy - y0) // h).astype(np.int64)
            order = np.argsort(cid, kind='stable')
            sx, sy, sv, cid = sx[order], sy[order], sv[order], cid[order]
            cell_start = np.searchsorted(cid, np.arange(ncx * ncy + 1)).astype(np.int32)
        else:
            x0 = y0 = 0.0; ncx = ncy = 1
            cell_start = np.zeros(2, dtype=np.int32)
        self.x0, self.y0, self.ncx, self.ncy, self.nsrc, self.sv = x0, y0, ncx, ncy, len(sx), sv
        f64 = np.dtype('float64')
        self.d_sx = ctx.to_device(sx if len(sx) else np.zeros(1), f64)
        self.d_sy = ctx.to_device(sy if len(sy) else np.zeros(1), f64)
        self.d_sv = ctx.to_device(np.ascontiguousarray(sv) if len(sx) else np.zeros((1, nf)), f64)
        self.d_cs = ctx.empty(cell_start.shape, np.int32).copy_from(cell_start)

    def interp(self, ctx, entry, d_tx, d_ty, ntarg, kernel_radius, sharpness):
        """`entry` (pgw_gauss_interp / pgw_gauss_interp_points) for every field, 16 per pass: (nfield, ntarg)."""
        f64 = np.dtype('float64')
        nf = self.nf
        out = np.empty((nf, ntarg))
        for k0 in range(0, nf, 16):                           # the kernel takes up to 16 fields per pass
            k1 = min(k0 + 16, nf)
            if k0 or k1 < nf:
                d_sub = ctx.to_device(np.ascontiguousarray(self.sv[:, k0:k1]), f64)
            else:
                d_sub = self.d_sv
            d_out = ctx.empty((k1 - k0, ntarg), f64)
            ctx._check(entry(ctx.handle, ntarg, d_tx.ptr, d_ty.ptr, self.ncx, self.ncy, self.x0, self.y0, self.h, self.d_cs.ptr,
                             self.nsrc, self.d_sx.ptr, self.d_sy.ptr, d_sub.ptr, k1 - k0, float(kernel_radius), float(sharpness),
                             d_out.ptr))
            out[k0:k1] = d_out.numpy()
        return out


def gauss_interp_fields(land_fr, era5_lat, era5_lon, gcm_lat, gcm_lon, fields, kernel_radius, sharpness):
    """The geometry and the GPU pass of nan_ignoring_interp for SEVERAL fields on the same source points (the twelve
    months of a variable: interp_wrapper calls nan_ignoring_interp once per month, functions.py:1102-1109, rebuilding
    the same two point clouds each time).
    land_fr (nlat, nlon); era5_lat (nlat), era5_lon (nlon); gcm_lat, gcm_lon, fields[k]: arrays of one common shape
    (curvilinear 2-D coordinates flattened like :931-933).  Returns (nfield, nlat, nlon) float64."""
    ctx = default_context()
    cloud = _OceanCloud(ctx, gcm_lat, gcm_lon, fields, kernel_radius)
    nf = cloud.nf
    elat = np.asarray(era5_lat, dtype=np.float64)
    elon = _fold_lon(era5_lon)
    tlat = np.repeat(elat, len(elon)); tlon = np.tile(elon, len(elat))                         # :1004-1005
    # lat_m depends on the latitude only, lon_m on (|lat|, |lon|): evaluate the distinct values of the regular grid once
    la_u, la_i = np.unique(np.abs(elat), return_inverse=True)
    lo_u, lo_i = np.unique(np.abs(elon), return_inverse=True)
    uu_lat, uu_lon = np.repeat(la_u, len(lo_u)), np.tile(lo_u, len(la_u))
    u_arc, u_lon, _ = planar_metres(uu_lat, uu_lon)
    lat_arc = u_arc.reshape(len(la_u), len(lo_u))[:, 0]
    lon_arc = u_lon.reshape(len(la_u), len(lo_u))
    tx = (lat_arc[la_i] * np.sign(elat))[:, None] * np.ones(len(elon))[None, :]
    ty = lon_arc[np.ix_(la_i, lo_i)] * np.sign(elon)[None, :]
    # the kernel stages the source cells a BLOCK of 256 consecutive targets needs, and a wave runs the weight arithmetic of a
    # source point when ANY of its 64 lanes has the point within the radius: hand the targets over in tiles of 16 x 16 grid
    # points (one block; a wave = 4 x 16 of them) instead of row by row - a compact footprint, so few cells per block and
    # few accepted points per wave that most of its lanes reject.  Edge tiles are filled with NaN (inactive) targets.
    nlat_t, nlon_t = tx.shape
    TILE = 16
    nlat_p, nlon_p = -(-nlat_t // TILE) * TILE, -(-nlon_t // TILE) * TILE

    # tiles of the high latitudes first: the planar cloud is densest there (a parallel shrinks, the points on it do not get
    # fewer), so those blocks run longest; started first they do not form the tail of the launch
    nty, ntx = nlat_p // TILE, nlon_p // TILE
    row_lat = np.abs(np.pad(elat, (0, nlat_p - nlat_t), mode='edge').reshape(nty, TILE)).mean(axis=1)
    tile_order = np.argsort(-np.repeat(row_lat, ntx), kind='stable')

    def tiles(a):
        full = np.full((nlat_p, nlon_p), np.nan)
        full[:nlat_t, :nlon_t] = a
        return full.reshape(nty, TILE, ntx, TILE).transpose(0, 2, 1, 3).reshape(nty * ntx, TILE * TILE)[tile_order]
    tx, ty = tiles(tx), tiles(ty)
    tx, ty = np.ascontiguousarray(tx.reshape(-1)), np.ascontiguousarray(ty.reshape(-1))
    f64 = np.dtype('float64')
    d_tx, d_ty = ctx.to_device(tx, f64), ctx.to_device(ty, f64)
    out = cloud.interp(ctx, ctx.lib.pgw_gauss_interp, d_tx, d_ty, len(tx), kernel_radius, sharpness)
    back = np.empty_like(tile_order)
    back[tile_order] = np.arange(len(tile_order))
    out = out.reshape(nf, nty * ntx, TILE * TILE)[:, back]
    out = out.reshape(nf, nty, ntx, TILE, TILE).transpose(0, 1, 3, 2, 4).reshape(nf, nlat_p, nlon_p)
    out = np.ascontiguousarray(out[:, :nlat_t, :nlon_t]).reshape(nf, -1)
    land = np.asarray(land_fr, dtype=np.float64).reshape(-1)
    out[:, land > 0.7] = np.nan                               # :1032, 1055: no SST on land points
    return out.reshape(nf, len(elat), len(elon))


def gauss_interp_points(land_fr, targ_lat, targ_lon, gcm_lat, gcm_lon, fields, kernel_radius, sharpness):
    """gauss_interp_fields for POINT-WISE targets: targ_lat / targ_lon [deg] of one common shape of rank >= 1 (2-D
    coordinates of a rotated-pole file, a cell list), land_fr of that shape or None.  The target side runs on the GPU:
    planar metres (`pgw_ocean_targets`: targets with land_fr > 0.7 or a NaN coordinate are inactive and come back NaN),
    then `pgw_gauss_interp_points`, which orders the targets by the source's cells on the device and writes every result
    to its own place.  A mesh handed over point by point gives the bits of gauss_interp_fields.
    Returns (nfield,) + targ_lat.shape float64."""
    tlat = np.asarray(targ_lat, dtype=np.float64)
    tlon = np.asarray(targ_lon, dtype=np.float64)
    if tlat.ndim < 1 or tlat.shape != tlon.shape:
        raise ValueError('target latitudes of shape %s and longitudes of shape %s must have one common shape of rank >= 1'
                         % (tlat.shape, tlon.shape))
    land = None if land_fr is None else np.asarray(land_fr, dtype=np.float64)
    if land is not None and land.shape != tlat.shape:
        raise ValueError('land fraction of shape %s does not lie on the targets of shape %s' % (land.shape, tlat.shape))
    ntarg = tlat.size
    if ntarg == 0:
        return np.empty((_ocean_source_values(gcm_lat, gcm_lon, fields)[2].shape[1],) + tlat.shape)
    _ocean_source_values(gcm_lat, gcm_lon, fields)            # its shape error comes before the context is touched
    ctx = default_context()
    cloud = _OceanCloud(ctx, gcm_lat, gcm_lon, fields, kernel_radius)
    f64 = np.dtype('float64')
    d_lat, d_lon = ctx.to_device(np.ascontiguousarray(tlat.reshape(-1)), f64), ctx.to_device(np.ascontiguousarray(tlon.reshape(-1)), f64)
    d_land = None if land is None else ctx.to_device(np.ascontiguousarray(land.reshape(-1)), f64)
    d_tx, d_ty = ctx.empty((ntarg,), f64), ctx.empty((ntarg,), f64)
    ctx._check(ctx.lib.pgw_ocean_targets(ctx.handle, ntarg, d_lat.ptr, d_lon.ptr, None if d_land is None else d_land.ptr,
                                         d_tx.ptr, d_ty.ptr))
    out = cloud.interp(ctx, ctx.lib.pgw_gauss_interp_points, d_tx, d_ty, ntarg, kernel_radius, sharpness)
    return out.reshape((cloud.nf,) + tlat.shape)


def _ocean_coords(da_delta):
    """Latitudes / longitudes of the ocean grid as arrays of the values' shape (functions.py:920-933).  The reference
    builds a meshgrid for 1-D coordinates and then overwrites it with the raw 1-D coordinates (:931-932), which cannot
    index the flattened values; the meshgrid (evidently intended) is used here."""
    lat = np.asarray(da_delta.coords[LAT_GCM_OCEAN])
    lon = np.asarray(da_delta.coords[LON_GCM_OCEAN])
    if lat.ndim == 2:
        return lat, lon
    if lat.ndim == 1:
        return np.meshgrid(lat, lon, indexing='ij')
    raise NotImplementedError()


def nan_ignoring_interp(da_era5_land_fr, da_delta, kernel_radius, sharpness):
    """Point-cloud interpolation of a 2-D ocean-grid field onto the ERA5 grid, ignoring NaN source points; land points
    (FR_LAND > 0.7) come back NaN.  reference functions.py:900-1060.  Labelled inputs like the reference's
    (`.values`, `.coords` with the ocean grid's `latitude` / `longitude`, ERA5 `lat` / `lon`)."""
    glat, glon = _ocean_coords(da_delta)
    tg = _Target.of(da_era5_land_fr.coords[LAT_ERA], da_era5_land_fr.coords[LON_ERA], da_era5_land_fr.dims)
    interp = gauss_interp_points if tg.points else gauss_interp_fields
    res = interp(np.asarray(da_era5_land_fr.values), tg.lat, tg.lon, glat, glon, [np.asarray(da_delta.values)], kernel_radius, sharpness)
    return res[0]


def _ocean_time_field(t):
    from . import ncio
    return ncio.Field(t.values, ('time',), {'time': t.values}, {k: v for k, v in t.attrs.items() if k not in ('units', 'calendar')}
                      if t.values.dtype.kind == 'M' else t.attrs)


def interp_wrapper(origin_grid, target_grid, var_name, i_use_xesmf=0,
                   nan_interp_kernel_radius=300000, nan_interp_sharpness=3):
    """Per-variable choice of the regridding scheme (reference functions.py:1062-1141).
    Atmospheric variables: bilinear on the GPU.  `tos` / `siconc` (ocean grid, NaN over land): the Gaussian-kernel
    point-cloud interpolation, all twelve months in one pass - onto a mesh (1-D lat and lon axes) through
    gauss_interp_fields, onto lat / lon over shared dimensions (rotated-pole extpar file, cell list; FR_LAND over those
    dimensions or with a leading time axis of 1) through gauss_interp_points, the result laid out over ('time',) + those
    dimensions with lat / lon as variables over them."""
    from . import ncio
    if var_name in ['tos', 'siconc']:
        land = target_grid['FR_LAND']
        tg = _Target.of(target_grid[LAT_ERA], target_grid[LON_ERA])
        land = np.asarray(land.values)
        if not tg.points:
            land = land[0]                                                         # target_grid["FR_LAND"][0,:,:]  :1097
        elif land.shape == (1,) + tg.lat.shape:                # an extpar file has no time axis: (1,) + tdims or tdims
            land = land[0]
        elif land.shape != tg.lat.shape:
            raise ValueError('FR_LAND of shape %s lies neither over the target coordinates of shape %s nor over one '
                             'time step of them' % (land.shape, tg.lat.shape))
        values = origin_grid[var_name]
        glat, glon = _ocean_coords(ncio.Field(values.values[0], values.dims[1:],
                                              {LAT_GCM_OCEAN: np.asarray(origin_grid[LAT_GCM_OCEAN].values),
                                               LON_GCM_OCEAN: np.asarray(origin_grid[LON_GCM_OCEAN].values)}))
        if values.shape[0] != 12:
            raise ValueError('could not broadcast input array: %s has %d time steps, the ocean-grid interpolation expects 12 months'
                             % (var_name, values.shape[0]))                         # result = np.empty((12, ...))  :1101
        interp = gauss_interp_points if tg.points else gauss_interp_fields
        result = interp(land, tg.lat, tg.lon, glat, glon, [values.values[i] for i in range(12)],
                        nan_interp_kernel_radius, nan_interp_sharpness)
        ds = ncio.Dataset(attrs=dict(description=str(var_name) + " on ERA5 grid", units="K", long_name=str(var_name)))   # :1121, 1134
        tg.put_coords(ds, target_grid[LAT_ERA].attrs, target_grid[LON_ERA].attrs)      # point-wise: as regrid_lat_lon lays them out
        ds['time'] = _ocean_time_field(origin_grid[TIME_GCM])
        tg.put_field(ds, var_name, result, ('time',), {'time': ds['time'].values})
        return ds
    return regrid_lat_lon(origin_grid, target_grid, var_name, method='bilinear', i_use_xesmf=i_use_xesmf)
