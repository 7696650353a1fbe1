"""
step_03: impose the climate deltas on ERA5 files and re-balance surface pressure, on MI355X.

Mirror of the reference's `step_03_apply_to_era.py` (same `pgw_for_era5` signature, same
command-line flags, `-p` = number of worker ranks) with the per-file compute path running as
HIP kernels on device-resident arrays:

    RELHUM = q->RH(QV, pa(PS), T)                       reference step_03:64-94
    sea ice / skin / soil temperature riders            :103-146
    ta, hur, ua, va: time-lerp + surface insert + ln-p interpolation + add      :155-173
    fixed-point loop on delta_ps until max|phi error| <= 0.15                   :182-319
    PS, T, QV, U, V, T_SKIN, T_SO, FR_SEA_ICE written back                      :369-378

The twelve monthly records of every delta live in HBM for the whole run (`DeltaSet`; ~10 GB
fp64 at 0.25 deg for ta,hur,ua,va,zg on plev19 - the reference re-reads them from disk for
every file and `zg` once per iteration, functions.py:203 / step_03:292).
"""
import ctypes as C
import datetime as _dt
import os

import numpy as np

from . import _lib
from . import settings as S
from ._lib import _dp
from .constants import CON_G, CON_RD   # noqa: F401
from .device import DeviceArray, default_context, dtype_tag, ptr


# ----------------------------------------------------------------------------------------
# time bracketing of load_delta (reference functions.py:224-283), host control logic
# ----------------------------------------------------------------------------------------
def _to_dt64(t):
    return np.datetime64(t).astype('datetime64[s]')


def _reyear(times, year):
    """`dt64_to_dt(t).replace(year=year)` of functions.py:235-238 for an array of stamps: month, day and time of day kept."""
    y = times.astype('datetime64[Y]')
    m = times.astype('datetime64[M]')
    month = (m - y.astype('datetime64[M]')).astype(np.int64)                     # 0 .. 11
    rest = times - m.astype('datetime64[s]')                                       # day of month and time of day
    first = (np.datetime64('%04d' % year, 'Y').astype('datetime64[M]') + month).astype('datetime64[s]')
    return first + rest


def delta_time_bracket(delta_times, target):
    """Indices and (re-yeared) stamps of the records bracketing `target`, periodic in the
    year; Feb-29 dropped first.  Returns (ind_before, ind_after, x_hi, x_new, keep) with
    x_* = float nanoseconds relative to the 'before' stamp (what xarray hands to scipy).
    Array arithmetic on datetime64 (a daily axis has 365 stamps and this runs in front of every file)."""
    times = np.asarray(delta_times).astype('datetime64[s]')
    target = _to_dt64(target)
    m = times.astype('datetime64[M]')
    month = (m - times.astype('datetime64[Y]').astype('datetime64[M]')).astype(np.int64)
    day = ((times - m.astype('datetime64[s]')).astype(np.int64)) // 86400        # 0-based day of the month
    is_leap_day = np.nonzero((month == 1) & (day == 28))[0]                       # :224-230: the LAST Feb 29 found is dropped
    leap = int(is_leap_day[-1]) if len(is_leap_day) else None
    keep = np.array([i for i in range(len(times)) if i != leap], dtype=np.int64)
    year = int(str(target)[:4])
    ty = _reyear(times[keep], year)                                               # :235-238
    before = ty <= target                                                         # :242-243
    if before.any():
        ib = int(np.nonzero(before)[0][-1]); tb = ty[ib]
    else:                                                                         # :253-258
        ib = len(ty) - 1; tb = _reyear(ty[ib:ib + 1], year - 1)[0]
    after = ty >= target                                                          # :262-263
    if after.any():
        ia = int(np.nonzero(after)[0][0]); ta = ty[ia]
    else:                                                                         # :273-278
        ia = 0; ta = _reyear(ty[:1], year + 1)[0]
    ns = 'datetime64[ns]'
    x_hi = float((ta.astype(ns) - tb.astype(ns)).astype(np.int64))
    x_new = float((target.astype(ns) - tb.astype(ns)).astype(np.int64))
    if ib == ia:                                                                  # :282-283
        x_hi = 0.0; x_new = 0.0
    return ib, ia, x_hi, x_new, keep


# ----------------------------------------------------------------------------------------
# deltas resident in HBM
# ----------------------------------------------------------------------------------------
class DeltaSet:
    """The climate deltas of one run on the device.

    arrays: dict var -> [nrec, (nplev,) nlat, nlon] for ta,hur,ua,va,zg (4-D) and tas,hurs,ts,tos,siconc,ps_hist (3-D): a
    host array, a DeviceArray, or a record provider (`ncio.RecordReader`: .nrec, .rec_shape, .read_record(r)).  A provider
    with `.device_record(r, out)` (`SourceRecords`: records of a delta on the GCM's grid, regridded on the device) fills a
    record's DeviceArray itself, in stream order; such a variable always keeps the window.  A provider with `.variables` and
    `.device_pair(r, out_a, out_b)` (`SourceWindRecords`: ua and va regridded and rotated in one launch) stands under both of
    its variables and fills record r of both at once: their windows hold the same records, in the same order.  `plev` in
    file order (descending for CMIP).

    Time axes: the reference loads every delta file on its own (load_delta, functions.py:195-303), so each variable has
    its own time axis - `times_by_var[var]`, default `delta_times` - and is bracketed on it (monthly tos / siconc beside
    daily 3-D deltas work).

    HBM budget rule: all records of all variables stay resident when they fit into `PGW_DELTA_HBM_FRACTION` (default
    0.35) of the device's memory - 12 monthly records of everything at 0.25 deg are 10 GB in float64.  Otherwise (365
    daily records of five 19-level variables: 288 GB in float64, 144 GB in float32) a variable keeps a window of
    `WINDOW` records on the device: consecutive ERA5 files need the same two, a new record is uploaded when the instant
    moves past one (least recently used record dropped).  resident=True / False forces either."""

    VARS_3D = ('ta', 'hur', 'ua', 'va', 'zg')
    VARS_2D = ('tas', 'hurs', 'ts', 'tos', 'siconc', 'ps_hist')
    WINDOW = 4

    def __init__(self, ctx, arrays, delta_times, plev, dtype, times_by_var=None, resident=None):
        self.ctx = ctx
        self.dtype = np.dtype(dtype)
        self.times = None if delta_times is None else np.asarray(delta_times).astype('datetime64[s]')
        self.plev = np.ascontiguousarray(plev, dtype=np.float64)
        self.plev_zg = self.plev                                    # zg_delta.nc may bring its own plev axis (load_delta_set)
        self.times_by_var = {}
        self.dev, self._src, self._cache, self._lock = {}, {}, {}, __import__('threading').Lock()
        names = [k for k in self.VARS_3D + self.VARS_2D if k in arrays]
        for k in names:
            t = (times_by_var or {}).get(k)
            t = self.times if t is None else np.asarray(t).astype('datetime64[s]')
            if t is None:
                raise ValueError('no time axis for %s' % k)
            if self._nrec(arrays[k]) != len(t):
                raise ValueError('time axis of %s has %d stamps, the array %d records' % (k, len(t), self._nrec(arrays[k])))
            self.times_by_var[k] = t
        if self.times is None and 'ta' in self.times_by_var:
            self.times = self.times_by_var['ta']
        # variables with equal time axes share one bracket computation per instant (the bracket is host work in front of
        # every file's one C call: a dozen of them per file cost 0.2 ms of a 3.4 ms file)
        self._axis_of, axes = {}, []
        for k, t in self.times_by_var.items():
            for i, u in enumerate(axes):
                if len(u) == len(t) and bool(np.all(u == t)):
                    self._axis_of[k] = i
                    break
            else:
                self._axis_of[k] = len(axes)
                axes.append(t)
        self._axes = axes
        self._bracket_cache = {}
        total = sum(self._nrec(arrays[k]) * self._rec_elems(arrays[k]) for k in names) * self.dtype.itemsize
        if resident is None:
            forced = os.environ.get('PGW_DELTA_RESIDENT')
            if forced in ('0', '1'):
                resident = forced == '1'
            else:
                resident = total <= self.budget_bytes(ctx)
        self.resident, self.total_bytes = bool(resident), int(total)
        for k in names:
            a = arrays[k]
            if isinstance(a, DeviceArray):
                self.dev[k] = a
            elif hasattr(a, 'device_record') or hasattr(a, 'device_pair'):
                self._src[k] = a
                self._cache[k] = {}
            elif self.resident:
                if hasattr(a, 'read_record'):
                    a = np.stack([a.read_record(r) for r in range(a.nrec)])
                self.dev[k] = ctx.to_device(np.ascontiguousarray(a, dtype=self.dtype), self.dtype)
            else:
                self._src[k] = a
                self._cache[k] = {}
        # annual-mean skin-temperature delta (step_03:134-136): depends on the delta file only
        if 'ts' in arrays:
            _, _, _, _, keep = delta_time_bracket(self.times_by_var['ts'], self.times_by_var['ts'][0])
            ts = arrays['ts']
            if isinstance(ts, DeviceArray):
                mean = ts.numpy()[keep].astype(np.float64).mean(axis=0)
            elif hasattr(ts, 'read_record'):
                mean = np.zeros(ts.rec_shape, dtype=np.float64)
                for r in keep:                                      # one record at a time: the file may not fit in host memory
                    mean += ts.read_record(int(r)).astype(np.float64)
                mean /= len(keep)
            else:
                mean = np.asarray(ts)[keep].astype(np.float64).mean(axis=0)
            self.ts_clim = ctx.to_device(mean.astype(self.dtype), self.dtype)
        else:
            self.ts_clim = None

    @staticmethod
    def _nrec(a):
        return int(a.nrec) if hasattr(a, 'rec_shape') else int(a.shape[0])

    @staticmethod
    def _rec_elems(a):
        shape = a.rec_shape if hasattr(a, 'rec_shape') else a.shape[1:]
        return int(np.prod(shape, dtype=np.int64))

    @staticmethod
    def budget_bytes(ctx):
        import ctypes
        free, total = ctypes.c_size_t(0), ctypes.c_size_t(0)
        ctx._check(ctx.lib.pgw_mem_info(ctx.handle, ctypes.byref(free), ctypes.byref(total)))
        return int(float(os.environ.get('PGW_DELTA_HBM_FRACTION', '0.35')) * total.value)

    def __contains__(self, var):
        return var in self.times_by_var

    def rec(self, var, r):
        """Record `r` of `var` on the device: a slab of the resident array, or the window's copy (uploaded now if absent)."""
        r = int(r)
        if var in self.dev:
            return self.dev[var].slab(r)
        with self._lock:
            cache = self._cache[var]
            src = self._src[var]
            if hasattr(src, 'device_pair'):
                # both windows in lockstep: a hit is a hit in both, a miss takes the least recently used slot of both and one
                # launch fills them (in stream order, as below) - the other variable's request for r is then a hit
                caches = [self._cache[v] for v in src.variables]
                if r not in cache:
                    slots = [c.pop(next(iter(c))) if len(c) >= self.WINDOW else self.ctx.empty(src.rec_shape, self.dtype) for c in caches]
                    src.device_pair(r, *slots)
                    for c, arr in zip(caches, slots):
                        c[r] = arr
                else:
                    for c in caches:
                        c[r] = c.pop(r)                             # most recently used last
                return cache[r]
            if r in cache:
                cache[r] = cache.pop(r)                             # most recently used last
                return cache[r]
            if hasattr(src, 'device_record'):
                # the provider writes the record on the context's stream: every kernel that reads the slot of the least
                # recently used record was launched on it before, so the slot is reused without a host synchronisation
                arr = cache.pop(next(iter(cache))) if len(cache) >= self.WINDOW else self.ctx.empty(src.rec_shape, self.dtype)
                src.device_record(r, arr)
                cache[r] = arr
                return arr
            host = src.read_record(r) if hasattr(src, 'read_record') else src[r]
            if len(cache) >= self.WINDOW:
                old = next(iter(cache))
                arr = cache.pop(old)                                # reuse the buffer of the least recently used record
                self.ctx.sync()                                     # no kernel may still read it
                arr.copy_from(np.ascontiguousarray(host, dtype=self.dtype))
            else:
                arr = self.ctx.to_device(np.ascontiguousarray(host, dtype=self.dtype), self.dtype)
            cache[r] = arr
            return arr

    def same_axis(self, var, ref='ta'):
        return self._axis_of[var] == self._axis_of[ref]

    def bracket(self, target, var=None):
        if var is None:
            return delta_time_bracket(self.times, target)
        key = (self._axis_of[var], target)
        hit = self._bracket_cache.get(key)
        if hit is None:
            if len(self._bracket_cache) > 64:
                self._bracket_cache.clear()
            hit = self._bracket_cache[key] = delta_time_bracket(self._axes[key[0]], target)
        return hit

    def pair(self, var, target, scratch):
        """(record before, record after, x_hi, x_new) of `var` for the instant, bracketed on its OWN time axis
        (functions.py:240-283).  x_hi == 0: the instant is a record (the 'after' record is the same array)."""
        ib, ia, x_hi, x_new, keep = self.bracket(target, var)
        return self.rec(var, keep[ib]), self.rec(var, keep[ia]), x_hi, x_new

    def pair_on_axis_of(self, var, target, main_x, scratch):
        """The pair of `var` for kernels that interpolate a group of variables with ONE (x_hi, x_new) = main_x, the
        bracket of `ta`: the records themselves when `var` shares ta's time axis, else `var` interpolated here on its own
        axis and handed over as both records (b + (b - b) / x_hi * x_new = b).  `scratch(name, shape)` supplies the buffer.
        (A float32 run holds that one field rounded to float32, where the fused path keeps the float64 value.)"""
        if self.same_axis(var):
            ib, ia, _, _, keep = self.bracket(target, 'ta')
            return self.rec(var, keep[ib]), self.rec(var, keep[ia])
        b, a, x_hi, x_new = self.pair(var, target, scratch)
        if x_hi == 0.0:
            return b, b
        out = scratch('_pre_' + var, b.shape)
        self.ctx._check(self.ctx.lib.pgw_time_lerp(self.ctx.handle, dtype_tag(self.dtype), b.size, b.ptr, a.ptr, x_hi, x_new,
                                                   out.ptr))
        return out, out

    def lerp2d(self, name, target, out=None):
        """Time-interpolated delta record (load_delta, functions.py:195-303) -> (1,) + record shape."""
        b, a, x_hi, x_new = self.pair(name, target, None)
        if out is None:
            out = self.ctx.empty((1,) + b.shape, self.dtype)
        if x_hi == 0.0:
            self.ctx._check(self.ctx.lib.pgw_memcpy_d2d(self.ctx.handle, out.ptr, b.ptr, b.nbytes))
        else:
            self.ctx._check(self.ctx.lib.pgw_time_lerp(self.ctx.handle, dtype_tag(self.dtype), b.size, b.ptr, a.ptr,
                                                       x_hi, x_new, out.ptr))
        return out

    def free(self):
        for v in list(self.dev.values()) + [x for c in self._cache.values() for x in c.values()] + [self.ts_clim]:
            if v is not None:
                v.free()
        for src in self._src.values():
            if hasattr(src, 'device_record') or hasattr(src, 'device_pair'):
                src.free()                                          # a paired provider is met twice: free() may be repeated
        self.dev, self._cache, self._src, self.ts_clim = {}, {}, {}, None


# Placement classes of the level arrays (device.SpreadPool; only their balance matters): the write streams
# of the quad kernel - T, e (the library's workspace: class 1, Context.enable_placement), U, V on the hybrid levels - two and two;
# the final kernel reads e (1) and writes QV (0); the inputs two and two.
LEVEL_CLASS_IN = {'T': 0, 'QV': 1, 'U': 0, 'V': 1}
LEVEL_CLASS_OUT = {'T': 0, 'QV': 0, 'U': 0, 'V': 1}


def _upload_era(ctx, era, dtype):
    out = {}
    for k in ('PS', 'FIS', 'T', 'QV', 'U', 'V', 'T_SKIN', 'T_SO', 'FR_LAND', 'FR_SEA_ICE'):
        v = era[k]
        if isinstance(v, DeviceArray):
            out[k] = v
        elif k in ('T', 'QV', 'U', 'V'):            # level fields: placed by the context (Context.level_array)
            h = np.ascontiguousarray(v, dtype=dtype)
            out[k] = ctx.level_array(h.shape, dtype, LEVEL_CLASS_IN[k]).copy_from(h)
        else:
            out[k] = ctx.to_device(np.ascontiguousarray(v, dtype=dtype), dtype)
    return out


def ref_dtype_mode(dtype, ref_dtype=None):
    """Whether a file of storage `dtype` runs in reference-dtype mode (settings.f32_file_mode; float32 files only)."""
    if np.dtype(dtype) != np.float32:
        if ref_dtype:
            raise ValueError('reference-dtype mode is the float32-file mode (float64 files already compute as the reference does)')
        return False
    if ref_dtype is None:
        if S.f32_file_mode not in ('reference', 'fast'):
            raise ValueError("settings.f32_file_mode must be 'reference' or 'fast'")
        return S.f32_file_mode == 'reference'
    return bool(ref_dtype)


def process_file_device(ctx, era, coeffs, deltas, target_dt, ignore_top_pressure_error=False,
                        p_ref=None, out=None, keep_hur=False, ref_dtype=None, i_reinterp=False):
    """The per-file compute path of pgw_for_era5 (reference step_03:62-346, i_reinterp = 0,
    fixed p_ref) on device arrays: ONE call into the C-ABI (`pgw_step03_file`).

    era: dict of DeviceArrays PS,FIS,(T_SKIN,FR_LAND,FR_SEA_ICE) (1,nlat,nlon); T,QV,U,V
    (1,N,nlat,nlon); T_SO (1,nsoil,nlat,nlon).  coeffs: dict ak,bk,[akm,bkm],soil1 (host).
    deltas: DeltaSet.  out: optional dict of preallocated output DeviceArrays (reused
    across files).  ref_dtype (float32 storage only; default settings.f32_file_mode): reference-dtype mode, T, QV, U, V
    come back as float64 arrays like the reference's `era + delta`.  i_reinterp: settings.i_reinterp = 1 (step_03:202-216,
    330-343: ta / hur and their deltas re-interpolated onto the current levels in every pass, ua / va after convergence) - the
    same call with `pgw_file_args.i_reinterp` set, every combination with the reference level and the storage modes.
    Returns (dict of DeviceArrays, info).

    Host side: with settings.file_plan (default) and reused `out` buffers, everything but the instant comes from a plan kept on
    the context and the library brackets the delta records itself (`pgw_step03_file_at`, _process_file_planned); otherwise, and
    wherever the plan does not cover the call, the argument struct is put together here for every file (_file_args)."""
    if p_ref is None:
        p_ref = S.p_ref_inp
    ref = ref_dtype_mode(deltas.dtype, ref_dtype)
    if out is not None and not keep_hur and _file_plan_on():
        done = _process_file_planned(ctx, era, coeffs, deltas, target_dt, ignore_top_pressure_error, p_ref, out, ref, i_reinterp)
        if done is not None:
            return done
    a, _held, out = _file_args(ctx, era, coeffs, deltas, target_dt, ignore_top_pressure_error, p_ref, out, keep_hur, ref, i_reinterp)
    ctx._last_file_args = a
    ctx._check(ctx.lib.pgw_step03_file(ctx.handle, C.byref(a)))
    return out, _file_info(a)


def _file_info(a):
    return dict(n_iter=a.n_iter, max_err=a.max_err_hist[:min(a.n_iter, 32)],
                levels_touched=int(a.levels_touched), passes_launched=int(a.passes_launched))


def _file_args(ctx, era, coeffs, deltas, target_dt, ignore_top_pressure_error, p_ref, out, keep_hur, ref, i_reinterp):
    """The `pgw_file_args` of one file put together on the host: every delta variable bracketed on its own time axis, output
    buffers drawn into `out` where they are missing.  Returns (args, what the args point into, out)."""
    local_p_ref = (p_ref is None) or (p_ref == 'local')          # settings.p_ref_inp = None, step_03:219-253
    dt = deltas.dtype
    ctx.set_levels(coeffs['ak'], coeffs['bk'], coeffs.get('akm'), coeffs.get('bkm'))
    T, PS = era['T'], era['PS']
    nt, N, nlat, nlon = T.shape
    if nt != 1:
        # the deltas are time-interpolated to ONE instant (functions.py:288-296); with more than one time step in
        # the file the reference fails in vert_interp_delta -> interp_logp_4d (functions.py:457-459)
        raise ValueError('Time dimension of input files is inconsistent!')
    out = {} if out is None else out
    dt4 = np.dtype('float64') if ref else dt                        # era (float32) + delta (float64), step_03:170-173

    def buf(name, shape, dtype=dt):
        if name not in out or out[name].shape != tuple(shape) or out[name].dtype != dtype:
            out[name] = ctx.level_array(shape, dtype, LEVEL_CLASS_OUT[name]) if name in LEVEL_CLASS_OUT else ctx.empty(shape, dtype)
        return out[name]

    _, _, x_hi, x_new, _ = deltas.bracket(target_dt, 'ta')          # functions.py:224-283, the axis of the quad group
    plev = deltas.plev
    a = _lib.FileArgs()
    a.per_var_time = 1                                              # every delta file is bracketed on its own time axis
    a.i_reinterp = 1 if i_reinterp else 0
    _lib.check_nplev(len(plev))                                     # before anything is copied or launched
    plev_zg = deltas.plev_zg
    if not (isinstance(plev_zg, np.ndarray) and plev_zg.dtype == np.float64 and plev_zg.flags.c_contiguous):
        plev_zg = deltas.plev_zg = np.ascontiguousarray(plev_zg, dtype=np.float64)       # once: the DeltaSet keeps the table
    if local_p_ref:
        _lib.check_nplev_zg(len(plev_zg))
    zb, za, a.zg_x_hi, a.zg_x_new = deltas.pair('zg', target_dt, buf)
    if local_p_ref:
        # the candidates for the reference level are zg's plev (step_03:219-222) and the zg delta is selected on that
        # axis (:292-295): it need not be the axis of ta / hur / ua / va (CFday: 99 levels against Emon / Amon's)
        if zb.shape[-3] != len(plev_zg):
            raise ValueError('the zg delta has %d levels, its plev axis %d' % (zb.shape[-3], len(plev_zg)))
        a.local_p_ref = 1
        a.zg3_b, a.zg3_a = zb.ptr, za.ptr
        a.nplev_zg = len(plev_zg)
        a.plev_zg = plev_zg.ctypes.data
    else:
        kref = np.nonzero(deltas.plev_zg == p_ref)[0]               # .sel(plev=p_ref), step_03:294
        if len(kref) != 1:
            raise KeyError(p_ref)
        a.zg_b = zb.slab(int(kref[0])).ptr
        a.zg_a = za.slab(int(kref[0])).ptr
        a.p_ref = float(p_ref)
    a.dtype, a.ntime, a.nlev, a.nplev, a.ncol = dtype_tag(dt), nt, N, len(plev), nlat * nlon
    a.ignore_top = 1 if ignore_top_pressure_error else 0
    a.ref_dtype = 1 if ref else 0
    a.max_n_iter = int(S.max_n_iter)
    a.adj_factor, a.thresh = float(S.adj_factor), float(S.thresh_phi_ref_max_error)
    a.x_hi, a.x_new = x_hi, x_new
    for k in ('PS', 'FIS', 'T', 'QV', 'U', 'V'):
        setattr(a, k, era[k].ptr)
    a.plev = plev.ctypes.data_as(_dp)
    held = []                                                       # keeps the record arrays alive until the call returns
    for var, name in (('ta', 'ta'), ('hur', 'hur'), ('ua', 'ua'), ('va', 'va'), ('tas', 'tas'), ('hurs', 'hurs'),
                      ('ps_hist', 'pshist')):
        b_, a_ = deltas.pair_on_axis_of(var, target_dt, (x_hi, x_new), buf)
        held += [b_, a_]
        setattr(a, name + '_b', b_.ptr)
        setattr(a, name + '_a', a_.ptr)
    held += [zb, za, plev, plev_zg]
    if 'FR_SEA_ICE' in era and 'siconc' in deltas:                  # surface riders, step_03:103-146
        soil = np.ascontiguousarray(coeffs['soil1'], dtype=np.float64)
        held.append(soil)
        a.nsoil = len(soil)
        a.soil_depth = soil.ctypes.data_as(_dp)
        for k in ('T_SKIN', 'T_SO', 'FR_LAND', 'FR_SEA_ICE'):
            setattr(a, k, era[k].ptr)
        for var in ('siconc', 'ts', 'tos'):
            b_, a_, vx_hi, vx_new = deltas.pair(var, target_dt, buf)
            held += [b_, a_]
            setattr(a, var + '_b', b_.ptr)
            setattr(a, var + '_a', a_.ptr)
            setattr(a, var + '_x_hi', vx_hi)
            setattr(a, var + '_x_new', vx_new)
        a.ts_clim = deltas.ts_clim.ptr
        a.T_SKIN_out = buf('T_SKIN', era['T_SKIN'].shape).ptr
        a.T_SO_out = buf('T_SO', era['T_SO'].shape).ptr
        a.FR_SEA_ICE_out = buf('FR_SEA_ICE', era['FR_SEA_ICE'].shape).ptr
    a.PS_out = buf('PS', PS.shape).ptr
    for k in ('T', 'QV', 'U', 'V'):
        setattr(a, k + '_out', buf(k, T.shape, dt4).ptr)
    if keep_hur:
        a.hur_pgw_out = buf('_hur_pgw', T.shape, dt4).ptr
    return a, held, out


# ----------------------------------------------------------------------------------------
# the file call from a plan: what stays from file to file is put together once per context
# ----------------------------------------------------------------------------------------
_ERA_NAMES = ('PS', 'FIS', 'T', 'QV', 'U', 'V', 'T_SKIN', 'T_SO', 'FR_LAND', 'FR_SEA_ICE')
_OUT_NAMES = ('PS', 'T', 'QV', 'U', 'V', 'T_SKIN', 'T_SO', 'FR_SEA_ICE')
_EPOCH = _dt.datetime(1970, 1, 1)
FILE_PLANS_KEPT = 8


def _file_plan_on():
    env = os.environ.get('PGW_FILE_PLAN')
    return bool(S.file_plan) if env is None else env != '0'


def _whole_seconds(t):
    """Seconds since 1970-01-01 of an instant without a sub-second part and without a time zone, else None."""
    if type(t) is _dt.datetime:
        if t.tzinfo is not None or t.microsecond:
            return None
        d = t - _EPOCH
        return d.days * 86400 + d.seconds
    try:
        t64 = np.datetime64(t)
        s = t64.astype('datetime64[s]')
        if np.isnat(s) or s != t64:
            return None
        return int(s.astype(np.int64))
    except (TypeError, ValueError):
        return None


def _array_key(arrays, names):
    return tuple([None if v is None else (v.ptr, v.shape, v.dtype) for v in map(arrays.get, names)])


class _FilePlan:
    """A `pgw_file_plan` and what it points into: the record arrays (through the DeltaSet), plev, soil1, the time axes."""

    def __init__(self, plan, deltas, held):
        self.plan, self.deltas, self.held = plan, deltas, held      # plan None: these arguments take the host-built struct
        self.ref = None if plan is None else C.byref(plan)


def _make_file_plan(ctx, era, coeffs, deltas, target_dt, ignore_top_pressure_error, p_ref, out, ref, i_reinterp):
    """The plan of this call, or None where the plan does not cover it: delta records not all resident, a member of the ta
    group on another time axis (it needs the pgw_time_lerp pre-pass of DeltaSet.pair_on_axis_of), anything _file_args
    refuses.  The template is the struct _file_args builds for this instant: the two host paths cannot drift apart."""
    riders = 'FR_SEA_ICE' in era and 'siconc' in deltas
    used = _lib.PLAN_VARS if riders else _lib.PLAN_VARS[:_lib.PLAN_QUAD_GROUP + 1]
    if any(var not in deltas.dev for var in used):
        return None
    if not all(deltas.same_axis(var) for var in _lib.PLAN_VARS[:_lib.PLAN_QUAD_GROUP]):
        return None
    if era['T'].shape[0] != 1:
        return None
    local_p_ref = (p_ref is None) or (p_ref == 'local')
    zg = deltas.dev['zg']
    if local_p_ref:
        ref_offset = 0                                              # the full records, on zg's own plev axis (args.plev_zg)
    else:
        kref = np.nonzero(deltas.plev_zg == p_ref)[0]
        if len(kref) != 1:
            return None
        ref_offset = int(kref[0]) * (zg.nbytes // (zg.shape[0] * zg.shape[1]))
    a, held, _ = _file_args(ctx, era, coeffs, deltas, target_dt, ignore_top_pressure_error, p_ref, out, False, ref, i_reinterp)
    plan = _lib.FilePlan()
    plan.args = a
    axes = {}
    for i, var in enumerate(used):                                  # `used` is a prefix of PLAN_VARS: i is the pgw_plan_var_id
        arr, ax = deltas.dev[var], deltas._axis_of[var]
        if ax not in axes:
            if len(axes) == _lib.PLAN_MAX_AXES:
                return None
            t = np.ascontiguousarray(deltas._axes[ax].astype('datetime64[s]').astype(np.int64))
            held.append(t)
            plan.axis_times[len(axes)] = t.ctypes.data_as(C.POINTER(C.c_longlong))
            plan.axis_len[len(axes)] = len(t)
            axes[ax] = len(axes)
        pv = plan.var[i]
        pv.base, pv.rec_bytes, pv.axis = arr.ptr, arr.nbytes // arr.shape[0], axes[ax]
        pv.ref_offset = ref_offset if var == 'zg' else 0
    plan.n_axes = len(axes)
    return _FilePlan(plan, deltas, held)


def _process_file_planned(ctx, era, coeffs, deltas, target_dt, ignore_top_pressure_error, p_ref, out, ref, i_reinterp):
    """process_file_device through the context's plan for these arguments: one C call.  None where the plan does not cover the
    call.  The key holds every value the template was built from (tests change `settings` between calls); the plans live on
    the Context, a few of them, least recently used dropped first (the command-line pipeline rotates a few buffer sets)."""
    target_s = _whole_seconds(target_dt)
    if target_s is None:
        return None
    soil1 = coeffs.get('soil1')

    def key_now():
        return (id(deltas), deltas.dtype, _array_key(era, _ERA_NAMES), _array_key(out, _OUT_NAMES), p_ref, ref, bool(i_reinterp),
                bool(ignore_top_pressure_error), S.max_n_iter, S.adj_factor, S.thresh_phi_ref_max_error,
                None if soil1 is None else np.asarray(soil1, dtype=np.float64).tobytes())

    plans = ctx._file_plans
    key = key_now()
    ent = plans.get(key)
    if ent is None or ent.deltas is not deltas:
        ent = (_make_file_plan(ctx, era, coeffs, deltas, target_dt, ignore_top_pressure_error, p_ref, out, ref, i_reinterp)
               or _FilePlan(None, deltas, None))
        plans.pop(key, None)
        plans[key_now()] = ent                                      # the output buffers may have been drawn just now
        while len(plans) > FILE_PLANS_KEPT:
            plans.popitem(last=False)
    else:
        plans.move_to_end(key)
    if ent.plan is None:
        return None
    ctx.set_levels(coeffs['ak'], coeffs['bk'], coeffs.get('akm'), coeffs.get('bkm'))
    a = _lib.FileArgs()
    ctx._last_file_args = a
    ctx._check(ctx.lib.pgw_step03_file_at(ctx.handle, ent.ref, target_s, C.byref(a)))
    return out, _file_info(a)


def process_file_device_reinterp(ctx, era, coeffs, deltas, target_dt, ignore_top_pressure_error=False,
                                 p_ref=None, out=None, ref_dtype=None, keep_hur=True):
    """settings.i_reinterp = 1 (reference step_03:202-216, 330-343): process_file_device with `i_reinterp` - ONE call into
    the C-ABI; fixed or local reference level, float64 / float32 files, reference-dtype mode."""
    return process_file_device(ctx, era, coeffs, deltas, target_dt, ignore_top_pressure_error, p_ref=p_ref, out=out,
                               keep_hur=keep_hur, ref_dtype=ref_dtype, i_reinterp=True)


def process_file_device_reinterp_composed(ctx, era, coeffs, deltas, target_dt, ignore_top_pressure_error=False,
                                          p_ref=None, out=None):
    """The same path composed on the host from the function-level C-ABI entries (pgw_reinterp_pass per pass,
    pgw_reinterp_pair for ua / va, the humidity entries) - round 2's form, fixed p_ref, float64 arithmetic on the storage
    type; kept as an independent composition the one-call path is tested against bit for bit."""
    lib, h = ctx.lib, ctx.handle
    p_ref = S.p_ref_inp if p_ref is None else p_ref
    if p_ref is None or p_ref == 'local':
        raise NotImplementedError('the host-composed form knows the fixed reference level only')
    dt = deltas.dtype
    tag = dtype_tag(dt)
    ctx.set_levels(coeffs['ak'], coeffs['bk'], coeffs.get('akm'), coeffs.get('bkm'))
    T, QV, PS, FIS = era['T'], era['QV'], era['PS'], era['FIS']
    nt, N, nlat, nlon = T.shape
    if nt != 1:
        raise ValueError('Time dimension of input files is inconsistent!')      # functions.py:457-459
    ncol, n2 = nlat * nlon, nt * nlat * nlon
    out = {} if out is None else out
    f64 = np.dtype('float64')

    def buf(name, shape, dtype=dt):
        if name not in out or out[name].shape != tuple(shape) or out[name].dtype != dtype:
            out[name] = ctx.empty(shape, dtype)
        return out[name]

    _, _, x_hi, x_new, _ = deltas.bracket(target_dt, 'ta')
    plev = deltas.plev
    # records of the group the kernels interpolate with ta's (x_hi, x_new); a variable on another time axis comes
    # interpolated on its own (DeltaSet.pair_on_axis_of)
    R = {var: deltas.pair_on_axis_of(var, target_dt, (x_hi, x_new), buf)
         for var in ('ta', 'hur', 'ua', 'va', 'tas', 'hurs', 'ps_hist')}
    kref = np.nonzero(deltas.plev_zg == p_ref)[0]
    if len(kref) != 1:
        raise KeyError(p_ref)
    # ERA state: RELHUM (step_03:87-94), phi_ref_era, g*dzg (the 4-D pressure fields live in registers, k_reinterp_field)
    relhum = buf('_RELHUM', T.shape)
    ctx._check(lib.pgw_specific_to_relative_humidity_hybrid(h, tag, nt, ncol, QV.ptr, PS.ptr, T.ptr, relhum.ptr))
    phi_era = buf('_phi_era', PS.shape, f64)
    ctx._check(lib.pgw_phi_ref_hybrid(h, tag, nt, ncol, T.ptr, QV.ptr, PS.ptr, FIS.ptr, float(p_ref), None, phi_era.ptr))
    dzg = buf('_dzg', PS.shape)
    zb, za, zx_hi, zx_new = deltas.pair('zg', target_dt, buf)                   # zg_delta.nc on its own time axis
    zb, za = zb.slab(int(kref[0])), za.slab(int(kref[0]))
    if zx_hi == 0.0:
        ctx._check(lib.pgw_memcpy_d2d(h, dzg.ptr, zb.ptr, zb.nbytes))
    else:
        ctx._check(lib.pgw_time_lerp(h, tag, zb.size, zb.ptr, za.ptr, zx_hi, zx_new, dzg.ptr))
    # loop state in buffers that live across files (a hipMalloc / hipFree per file synchronises the device)
    dphi = buf('_dphi', PS.shape, f64)
    dphi.copy_from(dzg.numpy().astype(np.float64) * CON_G)                        # step_03:292-293 (2-D, once)
    delta_ps, adj_ps = buf('_delta_ps', PS.shape, f64), buf('_adj_ps', PS.shape, f64)
    for x in (delta_ps, adj_ps):                                                  # :182-184
        ctx._check(lib.pgw_memset(h, x.ptr, 0, x.nbytes))
    ps_pgw = buf('PS', PS.shape)

    def reinterp_pair(var0, var1, era0, era1, target0, target1):
        """interp_logp_4d(era, pa_era, pa_pgw, 'constant') + load_delta_interp(var, pa_pgw)  :209-216 for two variables on
        the same axes (ta + hur: one ps_hist; ua + va), one kernel"""
        def arr(*ptrs):
            return (C.c_void_p * 2)(*[p.ptr if hasattr(p, 'ptr') else p for p in ptrs])
        if var0 in ('ta', 'hur'):
            sb = arr(R[var0 + 's'][0], R[var1 + 's'][0])
            sa = arr(R[var0 + 's'][1], R[var1 + 's'][1])
            pb, pa_ = R['ps_hist'][0].ptr, R['ps_hist'][1].ptr
        else:
            sb = sa = pb = pa_ = None
        ctx._check(lib.pgw_reinterp_pair(h, tag, nt, len(plev), ncol, plev.ctypes.data_as(_dp),
                                         arr(R[var0][0], R[var1][0]), arr(R[var0][1], R[var1][1]),
                                         x_hi, x_new, sb, sa, pb, pa_, arr(era0, era1), PS.ptr, ps_pgw.ptr,
                                         1 if ignore_top_pressure_error else 0, arr(target0, target1)))

    ta_pgw, hur_pgw = buf('T', T.shape), buf('_hur_pgw', T.shape)
    err = np.inf
    it = 1
    hist = []
    max_err = C.c_double()
    def arr(*xs):
        return (C.c_void_p * 2)(*[x.ptr for x in xs])
    thermo = (arr(R['ta'][0], R['hur'][0]), arr(R['ta'][1], R['hur'][1]), x_hi, x_new,
              arr(R['tas'][0], R['hurs'][0]), arr(R['tas'][1], R['hurs'][1]),
              R['ps_hist'][0].ptr, R['ps_hist'][1].ptr)
    while err > S.thresh_phi_ref_max_error:                                       # :189
        # one call and one host round trip per pass: delta_ps += adj_ps, ps_pgw (:192-193); ta / hur re-interpolated onto
        # the new levels (:202-216); the pass on them (:262-308)
        ctx._check(lib.pgw_reinterp_pass(h, tag, nt, len(plev), ncol, plev.ctypes.data_as(_dp), *thermo, T.ptr, relhum.ptr,
                                         PS.ptr, FIS.ptr, phi_era.ptr, dphi.ptr, delta_ps.ptr, adj_ps.ptr, float(p_ref),
                                         float(S.adj_factor), 1 if ignore_top_pressure_error else 0, ps_pgw.ptr, ta_pgw.ptr,
                                         hur_pgw.ptr, C.byref(max_err)))
        err = max_err.value                                                       # :308
        hist.append(err)
        it += 1
        if it > S.max_n_iter:                                                     # :313-319
            raise ValueError('ERROR! Pressure adjustment did not converge')
    reinterp_pair('ua', 'va', era['U'], era['V'], buf('U', T.shape), buf('V', T.shape))   # :330-343
    ctx._check(lib.pgw_relative_to_specific_humidity_hybrid(h, tag, nt, ncol, hur_pgw.ptr, ps_pgw.ptr, ta_pgw.ptr,
                                                            buf('QV', T.shape).ptr))   # hus of the last pass, :262-266,370
    if 'FR_SEA_ICE' in era and 'siconc' in deltas:                                # surface riders :103-146
        s3 = era['T_SKIN'].shape
        soil = np.ascontiguousarray(coeffs['soil1'], dtype=np.float64)
        ctx._check(lib.pgw_surface_update(
            h, tag, nt, ncol, len(soil), soil.ctypes.data_as(_dp), era['FR_SEA_ICE'].ptr,
            deltas.lerp2d('siconc', target_dt, buf('_dsic', s3)).ptr, deltas.lerp2d('tos', target_dt, buf('_dtos', s3)).ptr,
            deltas.lerp2d('ts', target_dt, buf('_dts', s3)).ptr, era['FR_LAND'].ptr, deltas.ts_clim.ptr,
            era['T_SKIN'].ptr, era['T_SO'].ptr, buf('FR_SEA_ICE', s3).ptr, buf('_dts_comb', s3).ptr,
            buf('T_SKIN', s3).ptr, buf('T_SO', era['T_SO'].shape).ptr))
    return out, dict(n_iter=it - 1, max_err=hist, levels_touched=0)


def _band_of(arrays, j0, j1):
    """Latitude rows [j0, j1) of every field of a dict (lat is the second-to-last axis; tables such as ak / bk pass through)."""
    out = {}
    for k, v in arrays.items():
        a = np.asarray(v) if v is not None else None
        out[k] = a[..., j0:j1, :] if (a is not None and a.ndim >= 3) else v
    return out


def pgw_for_era5_arrays(era, deltas, delta_times, plev, target_dt, ignore_top_pressure_error=False,
                        p_ref=None, dtype=None, i_reinterp=False, ref_dtype=None, band=None, reduce_max=None, resident=None,
                        plev_zg=None):
    """Whole-file path on in-memory host arrays (upload, compute on the GPU, download).

    plev (file order, 2 to 128 levels) is the axis of ta / hur / ua / va; plev_zg, when given, the axis of deltas['zg']
    (zg_delta.nc may come from another table: CFday ta beside Emon / Amon zg).  A fixed p_ref must be one of its levels;
    with p_ref = None / 'local' its levels (at most 64) are the candidates for the per-column reference level.

    band = (rank, world): this process handles latitude band `rank` of `world` of the file (parallel.band_rows) and
    returns that band's rows; `reduce_max` (parallel.band_max_hook) makes the loop's stopping test global, so the bands
    put together are bit for bit the single-process result, pass count and max|err| history included."""
    ctx = default_context()
    if band is not None:
        from .parallel import band_rows
        if i_reinterp:
            raise ValueError('latitude-band sharding of one file needs the multi-pass loop (settings.i_reinterp = 0)')
        if reduce_max is None and band[1] > 1:
            raise ValueError('band sharding over more than one rank needs reduce_max (parallel.band_max_hook)')
        j0, j1 = band_rows(np.asarray(era['T']).shape[-2], band[0], band[1])
        era, deltas = _band_of(era, j0, j1), _band_of(deltas, j0, j1)
    if reduce_max is not None:
        ctx.set_reduce_hook(reduce_max)
        try:
            return pgw_for_era5_arrays(era, deltas, delta_times, plev, target_dt, ignore_top_pressure_error, p_ref, dtype,
                                       i_reinterp, ref_dtype, resident=resident, plev_zg=plev_zg)
        finally:
            ctx.set_reduce_hook(None)
    if dtype is None:
        dtype = np.asarray(era['T']).dtype
    dtype = np.dtype(dtype)
    try:
        _lib.check_nplev(len(plev))
        if isinstance(delta_times, dict):                 # one time axis per delta file, like the reference's load_delta
            ds = DeltaSet(ctx, deltas, delta_times.get('ta'), plev, dtype, times_by_var=delta_times, resident=resident)
        else:
            ds = DeltaSet(ctx, deltas, delta_times, plev, dtype, resident=resident)
        if plev_zg is not None:
            ds.plev_zg = np.ascontiguousarray(plev_zg, dtype=np.float64)
        e = _upload_era(ctx, era, dtype)
        coeffs = dict(ak=era['ak'], bk=era['bk'], akm=era.get('akm'), bkm=era.get('bkm'), soil1=era['soil1'])
        if os.environ.get('PGW_TEST_FAIL_SETUP') == os.environ.get('RANK', '0') and ctx.has_reduce_hook():
            raise MemoryError('PGW_TEST_FAIL_SETUP: forced failure of the host-side set-up of this band')
    except BaseException:
        # latitude-band mode: the other bands are on their way into pgw_step03_file and would wait for this one in their
        # first reduce until the backend's timeout (gloo: 30 min) - tell them
        if ctx.has_reduce_hook():
            ctx.band_abort()
        raise
    if i_reinterp:
        out, info = process_file_device_reinterp(ctx, e, coeffs, ds, target_dt, ignore_top_pressure_error, p_ref,
                                                 ref_dtype=ref_dtype)
    else:
        out, info = process_file_device(ctx, e, coeffs, ds, target_dt, ignore_top_pressure_error, p_ref, keep_hur=True,
                                        ref_dtype=ref_dtype)
    res = {k: v.numpy() for k, v in out.items() if not k.startswith('_')}
    res['RELHUM_pgw'] = out['_hur_pgw'].numpy()
    res.update(info)
    return res


# ----------------------------------------------------------------------------------------
# file-level driver: pgw_for_era5 and the command line
# ----------------------------------------------------------------------------------------
_DELTASETS = {}


class _BandOfRecords:
    """A record provider cut to latitude rows [j0, j1) (band-wise runs with the record window)."""

    def __init__(self, reader, j0, j1):
        self.reader, self.j0, self.j1 = reader, j0, j1
        self.nrec = reader.nrec
        self.rec_shape = tuple(reader.rec_shape[:-2]) + (j1 - j0, reader.rec_shape[-1])

    def read_record(self, r):
        return self.reader.read_record(r)[..., self.j0:self.j1, :]


def delta_grid_mode(bands=False):
    """settings.delta_grid (PGW_DELTA_GRID, which the command line sets for the ranks it starts, overrides): 'era5' or
    'source', or 'source_points' (the deltas on the GCM's grid as for 'source', every column of the file a target of its own at
    its own lat / lon, whatever the file's layout), with what the two source values and settings.rotate_winds
    (PGW_ROTATE_WINDS likewise) exclude - all ValueErrors, raised before anything is read, copied or launched."""
    mode = os.environ.get('PGW_DELTA_GRID') or S.delta_grid
    if mode not in ('era5', 'source', 'source_points'):
        raise ValueError("settings.delta_grid must be 'era5' or 'source' (or 'source_points'), got %r" % (mode,))
    if mode != 'era5':
        if bands:
            raise ValueError("delta_grid = '%s' regrids whole records and does not run with --bands" % mode)
        if S.i_use_xesmf_regridding:
            raise ValueError("delta_grid = '%s' takes deltas on a regular lat / lon grid (the separable bilinear regridding); "
                             'with settings.i_use_xesmf_regridding = 1 run step_02 regridding and use the files it writes' % mode)
    rotate = rotate_winds_request()
    if rotate is not None:
        if mode == 'era5':
            raise ValueError("--rotate_winds with delta_grid = 'era5': the files under -d lie on the ERA5 grid already - rotate "
                             'in step_02 (`step_02 regridding --rotate_winds`), which writes them')
        if mode == 'source':
            raise ValueError("--rotate_winds with delta_grid = 'source': its targets are the mesh of 1-D lat / lon axes, whose "
                             "winds are geographic; a rotated-pole file takes delta_grid = 'source_points'")
        if rotate != 'auto':
            from .step_02_preproc_deltas import wind_pole
            wind_pole(rotate, None)                             # step_02's parsing errors
    return mode


def rotate_winds_request():
    """settings.rotate_winds (PGW_ROTATE_WINDS, which the command line sets for the ranks it starts, overrides): None - off -,
    'auto' or 'POLE_LAT,POLE_LON', as `step_02 regridding --rotate_winds` takes it."""
    return os.environ.get('PGW_ROTATE_WINDS') or S.rotate_winds


def _rotation_pole(era5, H):
    """The pole the winds are rotated about, or None: settings.rotate_winds read on the ERA5 Dataset by step_02's rule
    (`auto`: rotated_pole_of on the file's mapping).  ValueError on a mesh file, where there is nothing to rotate."""
    rotate = rotate_winds_request()
    if rotate is None:
        return None
    if is_mesh(H):
        raise ValueError('--rotate_winds: the file has 1-D %s / %s axes of their own - the winds of a lat-lon mesh are geographic '
                         'already, there is nothing to rotate' % (S.LAT_ERA, S.LON_ERA))
    from .step_02_preproc_deltas import wind_pole
    return wind_pole(rotate, era5)


class SourceRecords:
    """Record provider of a DeltaSet over one level variable of a delta file on the GCM's grid: record r is read and decoded
    like step_02 reads it (ncio.RecordReader: `_FillValue` / packing), uploaded into a staging buffer of one source record and
    regridded straight into the DeviceArray the DeltaSet hands over (functions.RegridPlan.apply onto a mesh,
    functions.PointsPlan.apply onto point-wise targets laid out as a grid: the bits of the regridded file cast to the
    DeltaSet's dtype) - all on the context's stream, nothing waits.  `rec_shape` is the regridded record's."""

    KEPT = 8                       # host records held after their upload was queued (each file call synchronises the stream)

    def __init__(self, ctx, reader, plan, *more_readers):
        self.ctx, self.reader, self.plan = ctx, reader, plan
        self.readers = (reader,) + more_readers
        self.nrec = int(reader.nrec)
        self.rec_shape = tuple(reader.rec_shape[:-2]) + tuple(plan.targ_shape)
        self.src_dtype = reader.dtype if reader.dtype in (np.dtype('float32'), np.dtype('float64')) else np.dtype('float64')
        self._stages = [None] * len(self.readers)
        self._held = __import__('collections').deque(maxlen=self.KEPT * len(self.readers))

    def _staged(self, k, r):
        """Record r of reader k, its upload into that reader's staging buffer queued on the stream."""
        host = np.ascontiguousarray(self.readers[k].read_record(int(r)), dtype=self.src_dtype)
        if self._stages[k] is None:
            self._stages[k] = self.ctx.empty(host.shape, self.src_dtype)
        self._held.append(host)
        self.ctx._check(self.ctx.lib.pgw_memcpy_h2d(self.ctx.handle, self._stages[k].ptr, host.ctypes.data, host.nbytes))
        return self._stages[k]

    def device_record(self, r, out):
        self.plan.apply(self._staged(0, r), out)
        return out

    def free(self):
        for k, st in enumerate(self._stages):
            if st is not None:
                st.free()                                       # waits for the stream
                self._stages[k] = None
        self._held.clear()
        self.plan.free()
        for reader in self.readers:
            reader.close()


class SourceWindRecords(SourceRecords):
    """The paired provider of ua and va on a rotated-pole file: record r of both files is uploaded and one
    functions.PointsPlan.apply_wind launch regrids and rotates them into the two DeviceArrays the DeltaSet hands over - the
    records of the files `step_02 regridding --rotate_winds` writes, cast to the DeltaSet's dtype.  The DeltaSet keeps the two
    windows in lockstep (DeltaSet.rec), so a record is read, uploaded and launched once for both variables."""

    variables = ('ua', 'va')
    device_record = None                                        # a record of one of the two alone is not to be had

    def __init__(self, ctx, reader_u, reader_v, plan):
        super().__init__(ctx, reader_u, plan, reader_v)

    def device_pair(self, r, out_u, out_v):
        self.plan.apply_wind(self._staged(0, r), self._staged(1, r), out_u, out_v)
        return out_u, out_v


def _open_era5_target(path):
    """The ERA5 file as step_02 opens its `-e` file, without the level fields: the axes and FR_LAND are what is needed."""
    from . import ncio
    vm = S.var_name_map
    return ncio.open_dataset(path, decode_times=False, skip=tuple(vm[k] for k in ('ta', 'hus', 'ua', 'va', 'st')))


def _mesh_axes(era5):
    """lat / lon of an ERA5 Dataset as float64 axes; ValueError unless they are 1-D axes of their own (a mesh)."""
    t_lat, t_lon = era5[S.LAT_ERA], era5[S.LON_ERA]
    if (len(t_lat.shape) != 1 or len(t_lon.shape) != 1 or tuple(t_lat.dims) != (S.LAT_ERA,) or tuple(t_lon.dims) != (S.LON_ERA,)):
        raise ValueError("delta_grid = 'source' needs an ERA5 file whose %s / %s are 1-D axes of their own; got %s over %s and %s "
                         'over %s' % (S.LAT_ERA, S.LON_ERA, t_lat.shape, tuple(t_lat.dims), t_lon.shape, tuple(t_lon.dims)))
    return np.asarray(t_lat.values, dtype=np.float64), np.asarray(t_lon.values, dtype=np.float64)


def _point_targets(era5):
    """(lat, lon, H) of an ERA5 Dataset for delta_grid = 'source_points': every column a target at its own position - float64
    arrays in the shape the file's fields go to the device in (era_layout: 2-D coordinates as they are, a cell list as a grid of
    one row, a mesh as the two axes meshed)."""
    from .functions import _Target
    H = era_layout(era5)
    tg = _Target.of(era5[S.LAT_ERA], era5[S.LON_ERA])
    if not tg.points:
        lat, lon = np.meshgrid(tg.lat, tg.lon, indexing='ij')
    else:
        lat, lon = _as_grid(tg.lat, H), _as_grid(tg.lon, H)
    return np.ascontiguousarray(lat), np.ascontiguousarray(lon), H


def _header_dataset(reader):
    """What functions.check_wind_pair asks of a delta file, from the header a RecordReader holds: the coordinates and the
    variable - dimensions, attributes, dtype - without its values."""
    from . import ncio
    ds = ncio.Dataset()
    for d, c in reader.coords.items():
        ds[d] = ncio.Field(np.asarray(c), (d,))
    ds[reader.var] = ncio.Field(ncio.placeholder((reader.nrec,) + tuple(reader.rec_shape), reader.dtype), tuple(reader.dims), {},
                                dict(reader.attrs))
    return ds


def check_source_wind_files(reader_u, reader_v):
    """The ua / va files of a rotating run, from their headers: functions.check_wind_pair (no marker of an earlier rotation,
    one source grid, plev, record count, dtype) and equal time axes - the two are served record by record together."""
    from .functions import check_wind_pair
    check_wind_pair(_header_dataset(reader_u), _header_dataset(reader_v), names=SourceWindRecords.variables)
    tu, tv = (np.asarray(r.coords.get(S.TIME_GCM, ())) for r in (reader_u, reader_v))
    if tu.shape != tv.shape or not bool(np.all(tu == tv)):
        raise ValueError('--rotate_winds: ua and va lie on different time axes; record r of both is regridded and rotated together')


def _load_source_delta_set(ctx, delta_input_dir, dtype, era5, mode='source'):
    """load_delta_set with delta_grid = 'source' / 'source_points': `delta_input_dir` holds what `step_02 regridding` takes as
    `-i`; the target is the mesh of the lat / lon axes of `era5` ('source'), or every column of it at its own lat / lon, by the
    file's own layout ('source_points': _point_targets; with settings.rotate_winds, ua / va come rotated onto the file's
    rotated grid through one paired provider).  `era5`: the path of the ERA5 file being processed, or (opened Dataset, path):
    the Dataset is asked for the coordinates, the file is opened like step_02's `-e` only when the deltas are not loaded yet."""
    from . import functions as F, ncio
    if era5 is None:
        raise ValueError("delta_grid = '%s' needs the ERA5 file whose lat / lon are the target" % mode)
    era5, era5_path = era5 if isinstance(era5, tuple) else (_open_era5_target(era5), None)
    pole = None
    if mode == 'source':
        (targ_lat, targ_lon), H = _mesh_axes(era5), (S.LAT_ERA, S.LON_ERA)
    else:
        targ_lat, targ_lon, H = _point_targets(era5)
        pole = _rotation_pole(era5, H)
    key = (os.path.abspath(delta_input_dir), np.dtype(dtype).str, ctx.device, None, mode, targ_lat.tobytes(), targ_lon.tobytes(), pole)
    if key in _DELTASETS:
        return _DELTASETS[key]
    if era5_path is not None:
        era5 = _open_era5_target(era5_path)
    base = S.file_name_bases
    readers = {var: ncio.RecordReader(os.path.join(delta_input_dir, base['SCEN-HIST'].format(var)), var) for var in DeltaSet.VARS_3D}
    times, plevs, plans, arrays = {}, {}, {}, {}
    try:
        for var, r in readers.items():
            if not r.dims or r.dims[0] != S.TIME_GCM or S.TIME_GCM not in r.coords:
                raise ValueError('%s: the first dimension of %s must be %s with a coordinate variable' % (r.path, r.var, S.TIME_GCM))
            if tuple(r.dims[-2:]) != (S.LAT_GCM, S.LON_GCM) or S.LAT_GCM not in r.coords or S.LON_GCM not in r.coords:
                raise ValueError('%s: %s must end in the dimensions (%s, %s), 1-D coordinates of their own'
                                 % (r.path, r.var, S.LAT_GCM, S.LON_GCM))
            times[var] = np.asarray(r.coords[S.TIME_GCM])
            plevs[var] = np.asarray(r.coords[S.PLEV_GCM], dtype=np.float64)
        plev = plevs['ta']
        for var in ('hur', 'ua', 'va'):
            if len(plevs[var]) != len(plev) or np.any(plevs[var] != plev):
                raise ValueError('plev axis of %s differs from that of ta (the four model-level deltas are interpolated together)' % var)
        if pole is not None:
            check_source_wind_files(readers['ua'], readers['va'])
        # one plan per source grid: regrid_tables runs here, the reference's extent errors come before any file is processed
        grids = {}
        for var, r in readers.items():
            lat, lon = np.asarray(r.coords[S.LAT_GCM], dtype=np.float64), np.asarray(r.coords[S.LON_GCM], dtype=np.float64)
            g = grids.setdefault((lat.tobytes(), lon.tobytes()), dict(lat=lat, lon=lon, nfield=1, vars=[]))
            g['nfield'] = max(g['nfield'], int(np.prod(r.rec_shape[:-2], dtype=np.int64)))
            g['vars'].append(var)
        for gkey, g in grids.items():
            if mode == 'source':
                plans[gkey] = F.RegridPlan(g['lat'], g['lon'], targ_lat, targ_lon, g['nfield'], ctx=ctx)
            else:
                winds = pole is not None and 'ua' in g['vars']
                plans[gkey] = F.PointsPlan(g['lat'], g['lon'], targ_lat, targ_lon, g['nfield'], pole=pole if winds else None, ctx=ctx)
            for var in g['vars']:
                if pole is not None and var in SourceWindRecords.variables:
                    if var == 'ua':
                        arrays['ua'] = arrays['va'] = SourceWindRecords(ctx, readers['ua'], readers['va'], plans[gkey])
                else:
                    arrays[var] = SourceRecords(ctx, readers[var], plans[gkey])
        # the surface deltas whole, by the calls of step_02 (step_02_preproc_deltas.main)
        surface = [(v, base['SCEN-HIST'].format(v), v) for v in ('tas', 'hurs', 'ts', 'tos', 'siconc')]
        for var, fname, name in surface + [('ps_hist', base['HIST'].format('ps'), 'ps')]:
            path = os.path.join(delta_input_dir, fname)
            if not os.path.exists(path):
                raise ValueError('Files for variable ' + name + ' are missing')
            out = F.interp_wrapper(ncio.open_dataset(path), era5, name, i_use_xesmf=0,
                                   nan_interp_kernel_radius=S.nan_interp_kernel_radius, nan_interp_sharpness=S.nan_interp_sharpness)
            f = out[name]
            if not f.dims or f.dims[0] != S.TIME_GCM or S.TIME_GCM not in f.coords:
                raise ValueError('%s: the first dimension of %s must be %s with a coordinate variable' % (path, name, S.TIME_GCM))
            if f.shape[0] > 365 + 1:
                raise ValueError('%s: %d records of %s; a surface delta stays on the device whole, a year of days at most'
                                 % (path, f.shape[0], name))
            arrays[var], times[var] = _as_grid(np.asarray(f.values), H), np.asarray(f.coords[S.TIME_GCM])
        dset = DeltaSet(ctx, arrays, times['ta'], plev, dtype, times_by_var=times, resident=True)
    except BaseException:
        for a in arrays.values():
            if hasattr(a, 'device_record'):
                a.free()                                        # the paired provider is met twice: free() may be repeated
        for pl in plans.values():
            pl.free()
        for r in readers.values():
            r.close()
        raise
    dset.plev_zg = plevs['zg']
    _DELTASETS[key] = dset
    return dset


def load_delta_set(ctx, delta_input_dir, dtype, band=None, era5=None):
    """All delta files of a directory -> DeltaSet on the device, cached per process (every ERA5 file of a run uses the
    same deltas).  Like the reference's load_delta (functions.py:195-303) every file brings its own time axis; the four
    model-level variables must share one plev axis (the quad kernel interpolates them together), zg may have its own.
    When all records fit the HBM budget (DeltaSet) the files are read whole; otherwise they are opened record-wise and
    the DeltaSet keeps a window of records per variable on the device.
    settings.delta_grid = 'source' / 'source_points': the directory holds the deltas on the GCM's grid and `era5` (path or
    opened Dataset of the ERA5 file being processed) gives the targets (_load_source_delta_set)."""
    from . import ncio
    mode = delta_grid_mode(bands=band is not None)
    if mode != 'era5':
        return _load_source_delta_set(ctx, delta_input_dir, dtype, era5, mode)
    key = (os.path.abspath(delta_input_dir), np.dtype(dtype).str, ctx.device, band)
    if key in _DELTASETS:
        return _DELTASETS[key]
    readers = {}
    for var in DeltaSet.VARS_3D + ('tas', 'hurs', 'ts', 'tos', 'siconc'):
        readers[var] = ncio.RecordReader(os.path.join(delta_input_dir, S.file_name_bases['SCEN-HIST'].format(var)), var)
    readers['ps_hist'] = ncio.RecordReader(os.path.join(delta_input_dir, S.file_name_bases['HIST'].format('ps')), 'ps')
    times, plevs = {}, {}
    for var, r in readers.items():
        if not r.dims or r.dims[0] != S.TIME_GCM or S.TIME_GCM not in r.coords:
            raise ValueError('%s: the first dimension of %s must be %s with a coordinate variable' % (r.path, r.var, S.TIME_GCM))
        times[var] = np.asarray(r.coords[S.TIME_GCM])
        if var in DeltaSet.VARS_3D:
            plevs[var] = np.asarray(r.coords[S.PLEV_GCM], dtype=np.float64)
    plev = plevs['ta']
    for var in ('hur', 'ua', 'va'):
        if len(plevs[var]) != len(plev) or np.any(plevs[var] != plev):
            raise ValueError('plev axis of %s differs from that of ta (the four model-level deltas are interpolated together)' % var)
    total = sum(r.nrec * int(np.prod(r.rec_shape, dtype=np.int64)) for r in readers.values()) * np.dtype(dtype).itemsize
    if band is not None:                                                        # (j0, j1): this rank's latitude rows
        nlat = readers['ta'].rec_shape[-2]
        total = total * (band[1] - band[0]) // max(nlat, 1)
    forced = os.environ.get('PGW_DELTA_RESIDENT')
    resident = (forced == '1') if forced in ('0', '1') else total <= DeltaSet.budget_bytes(ctx)
    # records over one horizontal dimension (step_02 wrote them onto a cell list): (plev, cell) is taken as (plev, 1, cell)
    cells = {var for var, r in readers.items() if len(r.rec_shape) == (2 if var in DeltaSet.VARS_3D else 1)}
    if cells and band is not None:
        for r in readers.values():
            r.close()
        raise ValueError('--bands on a point-wise file (deltas over a cell list) is not built')
    if resident:
        arrays = {}
        for var, r in readers.items():
            a = ncio.open_dataset(r.path)[r.var].values                         # whole file, threaded reads
            if var in cells:
                a = _as_grid(a, ('cell',))
            arrays[var] = a if band is None else np.ascontiguousarray(a[..., band[0]:band[1], :])
            r.close()
    elif cells:
        arrays = {k: _GridRecords(r) if k in cells else r for k, r in readers.items()}
    else:
        arrays = readers if band is None else {k: _BandOfRecords(r, band[0], band[1]) for k, r in readers.items()}
    dset = DeltaSet(ctx, arrays, times['ta'], plev, dtype, times_by_var=times, resident=resident)
    dset.plev_zg = plevs['zg']
    _DELTASETS[key] = dset
    return dset


_POOLS = {}
_BIG_OUT = ('T', 'QV', 'U', 'V')


# ----------------------------------------------------------------------------------------
# the horizontal layout of an ERA5 file
# ----------------------------------------------------------------------------------------
def _layout_of(lat_dims, lat_shape, lon_dims, lon_shape):
    from .functions import _target_layout
    points, dims = _target_layout(lat_dims, lat_shape, lon_dims, lon_shape)
    if not points:
        return (S.LAT_ERA, S.LON_ERA)
    if len(dims) > 2:
        raise ValueError('%s / %s over %s: the horizontal layout of a file has one dimension (a cell list) or two'
                         % (S.LAT_ERA, S.LON_ERA, dims))
    return tuple(dims)


def era_layout(ds):
    """The horizontal dimensions H of the fields of an ERA5 Dataset, by the rule of functions._target_layout on its
    settings.LAT_ERA / LON_ERA: (LAT_ERA, LON_ERA) where they are 1-D axes of their own (a mesh); their dimensions where
    both lie over the same one or two (2-D coordinates of a rotated-pole file: (rlat, rlon); a cell list: (cell,)); any
    other combination is the ValueError of _target_layout.  Every kernel of the per-file path works on independent columns:
    fields go to the device as (time, level, H0, H1), a cell list as a grid of one row (_as_grid).  A file without the two
    coordinate variables is the mesh it was taken for before there were layouts."""
    if S.LAT_ERA not in ds or S.LON_ERA not in ds:
        return (S.LAT_ERA, S.LON_ERA)
    lat, lon = ds[S.LAT_ERA], ds[S.LON_ERA]
    return _layout_of(lat.dims, lat.shape, lon.dims, lon.shape)


def file_layout(path):
    """era_layout from the header of the file at `path` (no field is read)."""
    from . import ncio
    got = []
    for name in (S.LAT_ERA, S.LON_ERA):
        try:
            r = ncio.RecordReader(path, name, decode_times=False)
        except KeyError:                                        # no such variable: a mesh, as era_layout takes it
            return (S.LAT_ERA, S.LON_ERA)
        got += [tuple(r.dims), (r.nrec,) + tuple(r.rec_shape)]
        r.close()
    return _layout_of(*got)


def is_mesh(H):
    return tuple(H) == (S.LAT_ERA, S.LON_ERA)


def layout_dims(H):
    """The dimension tuples of the 3-D, 4-D and soil fields of a file with horizontal dimensions H: dict d3, d4, so."""
    H = tuple(H)
    return dict(d3=(S.TIME_ERA,) + H, d4=(S.TIME_ERA, S.LEV_ERA) + H, so=(S.TIME_ERA, S.SOIL_HLEV_ERA) + H)


def _as_grid(v, H):
    """A field over (..., cell) as (..., 1, cell): a view of the same memory (a grid of one row); a field over two horizontal
    dimensions as it is."""
    return v.reshape(v.shape[:-1] + (1, v.shape[-1])) if len(H) == 1 else v


def _as_file(v, H):
    """The reverse of _as_grid: (..., 1, cell) back in the file's own shape (..., cell)."""
    return v.reshape(v.shape[:-2] + v.shape[-1:]) if len(H) == 1 else v


def _check_dims(name, field, dims, path=None):
    """ValueError where the field does not lie over exactly `dims` (a field of a point-wise file that lacks one of the
    horizontal dimensions), before anything is uploaded."""
    if sorted(field.dims) != sorted(dims):
        raise ValueError('%s%s lies over %s; the horizontal layout of the file asks for %s'
                         % ('' if path is None else path + ': ', name, tuple(field.dims), tuple(dims)))


class _GridRecords:
    """A record provider over a cell list, its records (..., cell) handed out as (..., 1, cell)."""

    def __init__(self, reader):
        self.reader, self.nrec = reader, reader.nrec
        self.rec_shape = tuple(reader.rec_shape[:-1]) + (1, reader.rec_shape[-1])

    def read_record(self, r):
        return self.reader.read_record(r).reshape(self.rec_shape)


def _io_raw():
    """PGW_IO_RAW=0 converts the byte order of the 4-D fields on the host (first version of the drivers);
    default: the file's big-endian bytes go to the GPU as they are, through pinned buffers, and come back
    big-endian, so no host pass touches a field between `pread` and `pwrite`."""
    return os.environ.get('PGW_IO_RAW', '1') != '0'


def _pinned_pool(ctx):
    from .device import PinnedPool
    with _BUFFER_LOCK:                              # the reader threads of the first two files arrive here together
        if id(ctx) not in _POOLS:
            _POOLS[id(ctx)] = PinnedPool(ctx)
        return _POOLS[id(ctx)]


def _release_pinned(pool, buf):
    """Give a pinned buffer back to the pool it came from; a buffer the pool does not know is a bug of the pipeline (it
    would never be recycled: 4.6 GB of pinned memory per float64 file), not something to pass over."""
    if not pool.release(buf):
        raise RuntimeError('a pinned buffer was released to a pool that does not own it')


def reset_after_abort():
    """parallel.run_shard calls this when a stage of the pipeline has failed and every stage thread has stopped: stage
    chains that were cancelled between two stages may have held a device buffer set or pinned buffers - all of them are free
    again, so that the next run in this process (a long-lived driver, a retry over the remaining files) finds them."""
    with _BUFFER_LOCK:
        for sets in _DEVICE_BUFFERS.values():
            sets.reset()
        for pool in _POOLS.values():
            pool.reclaim_all()
    _ABORT.clear()


def _stage_load(inp_era_file_path, out_era_file_path, delta_input_dir, era_step_dt,
                ignore_top_pressure_error, debug_mode=None):
    """Stage 1 (host, I/O): read one ERA5 file and lay its fields out as C-order host arrays."""
    from . import ncio
    if debug_mode is not None:
        raise NotImplementedError('debug_mode (step_03_apply_to_era.py:350-361, 387-414) is a validation aid of '
                                  'the reference and not part of the MI355X hot path')
    if S.f32_out_dtype not in ('float64', 'float32'):                  # checked before any buffer is taken
        raise ValueError("settings.f32_out_dtype must be 'float64' or 'float32'")
    delta_grid_mode()
    if S.i_debug >= 0:
        print('Start working on input file {}'.format(inp_era_file_path))
    raw = _io_raw()
    pinned = []
    alloc = None
    if raw:
        pool = _pinned_pool(default_context())

        def alloc(nbytes):
            buf = pool.acquire(nbytes)
            pinned.append(buf)
            return buf
    vm = S.var_name_map
    try:
        era_file = ncio.open_dataset(inp_era_file_path, decode_times=False, raw_big=raw, alloc=alloc)   # step_03:60
        H = era_layout(era_file)
        dims = layout_dims(H)
        if not is_mesh(H):
            for key, d in _FIELD_DIMS.items():
                _check_dims(vm[key], era_file[vm[key]], dims[d], inp_era_file_path)
    except BaseException:
        for b_ in pinned:
            _release_pinned(pool, b_)
        raise
    dtype = np.dtype('float64') if era_file[vm['ta']].dtype.itemsize == 8 else np.dtype('float32')
    dims3, dims4, dims_so = dims['d3'], dims['d4'], dims['so']

    def get(name, dims):
        v = era_file[name].transpose(*dims).values
        if (not v.dtype.isnative) and v.dtype.kind == 'f' and v.dtype.itemsize == dtype.itemsize and v.flags.c_contiguous:
            return _as_grid(v, H)                                            # file byte order; converted on the GPU
        return _as_grid(np.ascontiguousarray(v, dtype=dtype), H)

    era = dict(PS=get(vm['ps'], dims3), FIS=get(vm['zgs'], dims3), T=get(vm['ta'], dims4), QV=get(vm['hus'], dims4),
               U=get(vm['ua'], dims4), V=get(vm['va'], dims4), T_SKIN=get(vm['ts'], dims3),
               T_SO=get(vm['st'], dims_so), FR_LAND=get(vm['sftlf'], dims3), FR_SEA_ICE=get(vm['sic'], dims3))
    coeffs = dict(ak=np.asarray(era_file['ak'].values, dtype=np.float64), bk=np.asarray(era_file['bk'].values, dtype=np.float64),
                  soil1=np.asarray(era_file[S.SOIL_HLEV_ERA].values, dtype=np.float64))
    if 'akm' in era_file:                                                    # step_03:68-70
        coeffs['akm'] = np.asarray(era_file['akm'].values, dtype=np.float64)
        coeffs['bkm'] = np.asarray(era_file['bkm'].values, dtype=np.float64)
    return dict(era_file=era_file, era=era, coeffs=coeffs, dtype=dtype, out_path=out_era_file_path, inp_path=inp_era_file_path,
                delta_input_dir=delta_input_dir, era_step_dt=era_step_dt, ignore_top=ignore_top_pressure_error,
                dims=dims, layout=H, pinned=pinned)


class _BufferSets:
    """Device buffer sets of one (shape, dtype): `n` input sets and `n` output sets, handed round between the stages.
    With two sets the upload of file i+1 (stream 'h2d') and the download of file i-1 (stream 'd2h') run while the kernels
    of file i do - 288 GB of HBM hold many 0.25 deg L137 files (fp64: 4.6 GB in, 4.6 GB out each)."""

    def __init__(self, n):
        import queue
        self.inp, self.out = queue.Queue(), queue.Queue()
        self.all_inp, self.all_out = [{} for _ in range(n)], [{} for _ in range(n)]
        for a, b in zip(self.all_inp, self.all_out):
            self.inp.put(a)
            self.out.put(b)

    def reset(self):
        """all sets free again (after an aborted run: a cancelled stage chain may have held one)"""
        import queue
        for q, sets in ((self.inp, self.all_inp), (self.out, self.all_out)):
            while True:
                try:
                    q.get_nowait()
                except queue.Empty:
                    break
            for x in sets:
                q.put(x)


# the fields the per-file path reads (keys of settings.var_name_map) and the dimension tuple each lies over (layout_dims)
_FIELD_DIMS = dict(ps='d3', zgs='d3', ta='d4', hus='d4', ua='d4', va='d4', ts='d3', st='so', sftlf='d3', sic='d3')

_DEVICE_BUFFERS = {}
_BUFFER_LOCK = __import__('threading').Lock()
_ABORT = __import__('threading').Event()          # set by parallel.run_shard when a stage failed: waiting stages give up


def _buffer_sets(key):
    with _BUFFER_LOCK:
        if key not in _DEVICE_BUFFERS:
            _DEVICE_BUFFERS[key] = _BufferSets(max(1, int(os.environ.get('PGW_DEVICE_SETS', '2'))))
        return _DEVICE_BUFFERS[key]


def _take(q):
    """A free buffer set.  Gives up when another stage has failed (_ABORT) and - so that a set lost to a bug can never hang
    a run - after PGW_BUFFER_WAIT_S seconds (default 600; a stage of a 0.25 deg file takes well under a second)."""
    import queue
    import time
    t0 = time.time()
    limit = float(os.environ.get('PGW_BUFFER_WAIT_S', '600'))
    while True:
        try:
            return q.get(timeout=0.2)
        except queue.Empty:
            if _ABORT.is_set():
                raise RuntimeError('pipeline aborted: another stage failed')
            if time.time() - t0 > limit:
                raise RuntimeError('no device buffer set became free within %.0f s (PGW_BUFFER_WAIT_S)' % limit)


def _stage_upload(item):
    """Stage 2 (stream 'h2d'): host -> device copies of one file into a free input buffer set; the file's big-endian
    bytes are converted on the device."""
    ctx = default_context()
    up = ctx.side('h2d')
    dtype = item['dtype']
    item['deltas'] = load_delta_set(ctx, item['delta_input_dir'], dtype, era5=(item['era_file'], item['inp_path']))
    sets = _buffer_sets((item['era']['T'].shape, dtype.str))
    with _BUFFER_LOCK:                              # once per process and grid: where the level arrays of the buffer sets lie
        ctx.enable_placement(int(np.prod(item['era']['T'].shape, dtype=np.int64)) * 8, 8 * len(sets.all_inp) + 1)
    inp = _take(sets.inp)
    item['sets'], item['inp_set'] = sets, inp
    try:
        for k, v in item['era'].items():
            if k not in inp:
                inp[k] = ctx.level_array(v.shape, dtype, LEVEL_CLASS_IN[k]) if k in LEVEL_CLASS_IN else ctx.empty(v.shape, dtype)
            inp[k].copy_from(v, sync=False, ctx=up)
        up.sync()                                           # the host copies may go, and the compute stream may read
    except BaseException:
        sets.inp.put(inp)
        raise
    item['era'] = None                                      # release the host copies of the inputs
    return item


def _stage_compute(item):
    """Stage 3 (the context's own stream): one pgw_step03_file call on the uploaded buffers into a free output set."""
    ctx = default_context()
    sets, inp = item['sets'], item['inp_set']
    try:
        out_set = _take(sets.out)
    except BaseException:
        sets.inp.put(inp)
        raise
    try:
        out, info = process_file_device(ctx, inp, item['coeffs'], item['deltas'], item['era_step_dt'], item['ignore_top'],
                                        p_ref='local' if S.p_ref_inp is None else S.p_ref_inp, out=out_set,
                                        i_reinterp=bool(S.i_reinterp))
        ctx.sync()                                          # outputs complete before the 'd2h' stream reads them
    except ValueError as e:
        sets.out.put(out_set)
        if getattr(e, 'status', None) == _lib.PGW_ERR_NOT_CONVERGED or str(e).startswith('ERROR! Pressure adjustment did not converge'):
            raise ValueError('ERROR! Pressure adjustment did not converge ' +                   # step_03:315-319, text and file name
                             'for file {}. '.format(item.get('inp_path')) +
                             'Consider increasing the value for "max_n_iter" in ' +
                             'settings.py') from None
        raise
    except BaseException:
        sets.out.put(out_set)
        raise
    finally:
        sets.inp.put(inp)                                   # the next upload may overwrite the inputs
        item['inp_set'] = None
    item['out_set'], item['out'], item['info'], item['deltas'] = out_set, out, info, None
    if S.i_debug >= 2:
        for it, err in enumerate(info['max_err']):
            print('### iteration {:03d}, phi max error: {}'.format(it + 1, err))
    return item


def _stage_download(item):
    """Stage 4 (stream 'd2h'): results to the host - the large fields converted to the file's byte order on the device
    and DMA-ed into pinned buffers the writer `pwrite`s from."""
    from . import ncio
    ctx = default_context()
    dn = ctx.side('d2h')
    sets, out_set, out = item['sets'], item['out_set'], item['out']
    raw = _io_raw()
    pool = _pinned_pool(ctx) if raw else None
    result, pinned_out = {}, []
    # settings.f32_out_dtype = 'float32': the float64 T, QV, U, V of a float32 file leave the device as float32
    narrow = (S.f32_out_dtype == 'float32' and item['dtype'] == np.dtype('float32'))
    try:
        for k in ('PS', 'T', 'QV', 'U', 'V', 'T_SKIN', 'T_SO', 'FR_SEA_ICE'):
            o = out[k]
            if narrow and k in _BIG_OUT and o.dtype == np.dtype('float64'):
                sk = '_f32_' + k
                if sk not in out_set or out_set[sk].size != o.size:
                    out_set[sk] = ctx.empty(o.shape, np.float32)
                if raw and out_set[sk].nbytes >= ncio.BIG_VARIABLE:
                    hb = pool.acquire(out_set[sk].nbytes)
                    pinned_out.append(hb)
                    result[k] = o.download_narrow_f32(hb, out_set[sk], big_endian=True, ctx=dn)
                else:
                    hb = np.empty(out_set[sk].nbytes, dtype=np.uint8)
                    result[k] = o.download_narrow_f32(hb, out_set[sk], big_endian=False, ctx=dn)
            elif raw and k in _BIG_OUT and o.nbytes >= ncio.BIG_VARIABLE:
                hb = pool.acquire(o.nbytes)
                pinned_out.append(hb)
                result[k] = o.download_foreign(hb, ctx=dn)      # big-endian on the device, DMA into pinned memory
            else:
                result[k] = o.numpy(ctx=dn)
        dn.sync()
    except BaseException:
        for b_ in pinned_out:
            _release_pinned(pool, b_)
        raise
    finally:
        sets.out.put(out_set)
        item['out_set'] = item['out'] = None
    item['result'] = result
    # the four replaced 4-D variables leave the dataset now, so their pinned input buffers can be recycled
    # before the writer gets to this file
    era_file, vm = item['era_file'], S.var_name_map
    if pool is not None:
        for k in _BIG_OUT:
            old = era_file[vm[dict(T='ta', QV='hus', U='ua', V='va')[k]]]
            base = old.values
            old.values = np.empty((0,) * base.ndim, dtype=base.dtype)
            keep = []
            for b_ in item['pinned']:
                if b_.ctypes.data == base.ctypes.data:
                    _release_pinned(pool, b_)
                else:
                    keep.append(b_)
            item['pinned'] = keep
    item['pinned_out'] = pinned_out
    return item


def _stage_store(item):
    """Stage 3 (host, I/O): write the modified file (step_03:369-378: PS, T, QV, U, V; T_SKIN, T_SO and
    FR_SEA_ICE were updated in place at :105-144; RELHUM is never added)."""
    from . import ncio
    era_file, vm, d = item['era_file'], S.var_name_map, item['dims']
    names = dict(PS=(vm['ps'], d['d3']), T=(vm['ta'], d['d4']), QV=(vm['hus'], d['d4']), U=(vm['ua'], d['d4']),
                 V=(vm['va'], d['d4']), T_SKIN=(vm['ts'], d['d3']), T_SO=(vm['st'], d['so']), FR_SEA_ICE=(vm['sic'], d['d3']))
    try:
        for key, (name, dims) in names.items():
            old = era_file[name]
            era_file[name] = ncio.Field(_as_file(item['result'][key], item['layout']), dims,
                                        {k: old.coords[k] for k in dims if k in old.coords}, old.attrs)
        ncio.to_netcdf(era_file, item['out_path'])
    finally:
        bufs = item.get('pinned', []) + item.get('pinned_out', [])
        if bufs:
            pool = _pinned_pool(default_context())
            item['result'] = None
            for b_ in bufs:
                _release_pinned(pool, b_)
            item['pinned'], item['pinned_out'] = [], []
    if S.i_debug >= 1:
        print('Done. Saved to file {}.'.format(item['out_path']))
    return item['info']['n_iter']


def pgw_for_era5(inp_era_file_path, out_era_file_path, delta_input_dir, era_step_dt,
                 ignore_top_pressure_error, debug_mode=None):
    """Apply the PGW deltas to one ERA5 file (reference step_03_apply_to_era.py:44-381).
    Returns the number of loop passes.  When many files are processed through IterMP the three
    stages below run as a pipeline (read of file i+1 and write of file i-1 overlap the GPU work of
    file i; SURVEY.md section 8 f rank 1).
    debug_mode = 'interpolate_full' (step_03:350-361): the same computation, then the seven deltas are written instead of
    the ERA5 file - step_03_debug.debug_interpolate_full, synchronous, outside the stages (which refuse a debug mode)."""
    if debug_mode == 'interpolate_full':
        from .step_03_debug import debug_interpolate_full
        return debug_interpolate_full(inp_era_file_path, out_era_file_path, delta_input_dir, era_step_dt,
                                      ignore_top_pressure_error, debug_mode)
    return _stage_store(_stage_download(_stage_compute(_stage_upload(_stage_load(
        inp_era_file_path, out_era_file_path, delta_input_dir, era_step_dt, ignore_top_pressure_error, debug_mode)))))


def _no_bands_on_points(path):
    """`--bands` cuts latitude rows of a mesh: ValueError for a point-wise file, from its header, before a field is read."""
    H = file_layout(path)
    if not is_mesh(H):
        raise ValueError('--bands on a point-wise file is not built: %s has %s / %s over %s (latitude bands are rows of a mesh)'
                         % (path, S.LAT_ERA, S.LON_ERA, H))


def pgw_for_era5_banded(inp_era_file_path, out_era_file_path, delta_input_dir, era_step_dt, ignore_top_pressure_error,
                        rank, world, reduce_max, barrier):
    """ONE ERA5 file over `world` ranks in latitude bands (the latency mode) from file to file:
    every rank `pread`s its rows of the fields (ncio.read_band: one byte range per (time, level) plane of the classic
    layout), runs the per-file path on its band with the loop's stopping test made global by `reduce_max`
    (parallel.band_max_hook: MAX all-reduce of the per-pass figures), and `pwrite`s its rows into the shared output file
    whose header and remaining variables rank 0 wrote (ncio.BandedWriter).  The file equals the one-rank file byte for
    byte.  Every rank returns the pass count.  `barrier`: a callable all ranks meet in."""
    from . import ncio
    from .parallel import band_rows
    delta_grid_mode(bands=True)
    _no_bands_on_points(inp_era_file_path)
    if S.i_reinterp:
        raise ValueError('latitude-band sharding of one file needs the multi-pass loop (settings.i_reinterp = 0)')
    if S.f32_out_dtype not in ('float64', 'float32'):
        raise ValueError("settings.f32_out_dtype must be 'float64' or 'float32'")
    vm = S.var_name_map
    big = dict(T=vm['ta'], QV=vm['hus'], U=vm['ua'], V=vm['va'], PS=vm['ps'], T_SKIN=vm['ts'], T_SO=vm['st'], FR_SEA_ICE=vm['sic'])
    ctx = default_context()
    ctx.set_reduce_hook(reduce_max)
    try:
        try:
            if S.i_debug >= 0 and rank == 0:
                print('Start working on input file {} in {} latitude bands'.format(inp_era_file_path, world))
            ds = ncio.open_dataset(inp_era_file_path, decode_times=False, skip=tuple(big.values()))      # step_03:60
            dims4 = (S.TIME_ERA, S.LEV_ERA, S.LAT_ERA, S.LON_ERA)
            dims3 = (S.TIME_ERA, S.LAT_ERA, S.LON_ERA)
            for k, name in big.items():
                want = dims4 if k in ('T', 'QV', 'U', 'V') else ((S.TIME_ERA, S.SOIL_HLEV_ERA, S.LAT_ERA, S.LON_ERA) if k == 'T_SO' else dims3)
                if ds[name].dims != want:
                    raise NotImplementedError('band-wise I/O reads %s in the order %s, the file stores %s' % (name, want, ds[name].dims))
            dtype = np.dtype('float64') if ds[big['T']].dtype.itemsize == 8 else np.dtype('float32')
            nlat = ds[big['T']].shape[-2]
            j0, j1 = band_rows(nlat, rank, world)
            era = {k: np.ascontiguousarray(ncio.read_band(inp_era_file_path, name, j0, j1), dtype=dtype) for k, name in big.items()}
            for k, name in (('FIS', vm['zgs']), ('FR_LAND', vm['sftlf'])):                               # small: read whole
                era[k] = np.ascontiguousarray(ds[name].transpose(*dims3).values[..., j0:j1, :], dtype=dtype)
            coeffs = dict(ak=np.asarray(ds['ak'].values, dtype=np.float64), bk=np.asarray(ds['bk'].values, dtype=np.float64),
                          soil1=np.asarray(ds[S.SOIL_HLEV_ERA].values, dtype=np.float64))
            if 'akm' in ds:                                                                              # step_03:68-70
                coeffs['akm'] = np.asarray(ds['akm'].values, dtype=np.float64)
                coeffs['bkm'] = np.asarray(ds['bkm'].values, dtype=np.float64)
            deltas = load_delta_set(ctx, delta_input_dir, dtype, band=(j0, j1), era5=inp_era_file_path)
            e = _upload_era(ctx, era, dtype)
        except BaseException:
            ctx.band_abort()                  # the other bands are on their way into the loop's first reduce: tell them
            raise
        out, info = process_file_device(ctx, e, coeffs, deltas, era_step_dt, ignore_top_pressure_error,
                                        p_ref='local' if S.p_ref_inp is None else S.p_ref_inp)
        res = {k: out[k].numpy() for k in big}
        for v in list(e.values()) + [x for x in out.values()]:
            v.free()
    finally:
        ctx.set_reduce_hook(None)
    narrow = (S.f32_out_dtype == 'float32' and dtype == np.dtype('float32'))
    F = ncio.Field
    for k, name in big.items():
        old = ds[name]
        dt_out = res[k].dtype
        if narrow and k in _BIG_OUT:
            res[k] = res[k].astype(np.float32)                                  # the reference's float64 field rounded once
            dt_out = np.dtype('float32')
        ds[name] = F(ncio.placeholder(old.shape, dt_out), old.dims, old.coords, old.attrs)
    writer = ncio.BandedWriter(ds, out_era_file_path, tuple(big.values()))
    if rank == 0:
        writer.create()
    barrier()
    for k, name in big.items():
        writer.write_band(name, j0, j1, res[k])
    barrier()
    if S.i_debug >= 1 and rank == 0:
        print('Done. Saved to file {}.'.format(out_era_file_path))
    return info['n_iter']


pgw_for_era5.stages = (_stage_load, _stage_upload, _stage_compute, _stage_download, _stage_store)
pgw_for_era5.abort = _ABORT
pgw_for_era5.reset = reset_after_abort


def _cli(argv=None):
    import argparse
    p = argparse.ArgumentParser(description='Perturb ERA5 files with PGW climate deltas on MI355X GPUs '
                                            '(flags of the reference step_03_apply_to_era.py:505-568; settings in settings.py).')
    p.add_argument('-i', '--input_dir', type=str, default=None, help='directory with the ERA5 input files')
    p.add_argument('-o', '--output_dir', type=str, default=None, help='directory for the processed ERA5 files')
    p.add_argument('-f', '--first_era_step', type=str, default='2006080200', help='first time step, YYYYMMDDHH')
    p.add_argument('-l', '--last_era_step', type=str, default='2006080300', help='last time step (inclusive), YYYYMMDDHH')
    p.add_argument('-H', '--hour_inc_step', type=int, default=3, help='hours between time steps')
    p.add_argument('-d', '--delta_input_dir', type=str, default=None,
                   help='directory with the regridded climate deltas (output of step_02) and ps_historical.nc')
    p.add_argument('-p', '--n_par', type=int, default=1, help='number of worker ranks = GPUs; files are dealt round-robin')
    p.add_argument('-t', '--ignore_top_pressure_error', action='store_true',
                   help='do not fail if ERA5 reaches higher than the climate deltas')
    p.add_argument('-D', '--debug_mode', type=str, default=None,
                   help='write the climate deltas instead of the ERA5 files, to compare with the reference\'s -D output '
                        '(tools/compare_deltas.py).  interpolate_time: every delta interpolated in time only, '
                        'delta_{var}_{file} for tos, tas, hurs, ps, ta, hur, ua, va, zg (step_03_apply_to_era.py:387-414).  '
                        'interpolate_full: the deltas the run adds, on the model levels, {VAR}_delta_{file} for PS, T, RELHUM, '
                        'U, V, T_SO, T_SKIN (:350-361).  NetCDF-3 files beside the output path; one file at a time per rank; '
                        'not with --bands')
    p.add_argument('--delta_grid', type=str, default=None, choices=['era5', 'source', 'source_points'],
                   metavar='{era5,source}|source_points',
                   help="the grid of the deltas under -d (default: settings.delta_grid).  era5: the files step_02 regridding wrote.  "
                        'source: the files step_02 regridding takes as -i, on the GCM\'s regular lat / lon grid - regridded on the GPU '
                        'as they are needed, no intermediate files, the same output bytes; the ERA5 files have 1-D lat / lon axes.  '
                        'source_points: the same for ERA5 files of any layout (2-D lat / lon of a rotated-pole file, a cell list, a '
                        'mesh): every column is a target at its own lat / lon.  Neither with --bands.')
    p.add_argument('--rotate_winds', type=str, nargs='?', const='auto', default=None, metavar='auto|POLE_LAT,POLE_LON',
                   help='with --delta_grid source_points on a rotated-pole file: the ua / va deltas are turned onto the grid-relative '
                        'components (along rlon / rlat) the file stores, as `step_02 regridding --rotate_winds` writes them.  auto (the '
                        "value when none is given): the pole is taken from the file's rotated_latitude_longitude mapping; or the "
                        "geographic position of the grid's north pole in degrees.  Default: settings.rotate_winds (off)")
    p.add_argument('--bands', action='store_true',
                   help='latency mode: EVERY file is split over all ranks in latitude bands (each rank reads, computes and '
                        'writes its rows; one MAX all-reduce per loop launch) instead of file i -> rank i mod W.  Needs the '
                        'ranks of `python -m torch.distributed.run --nproc-per-node W -m pgw4era5_amd.step_03_apply_to_era ...`; '
                        'settings.i_reinterp = 0.  No counterpart in the reference.')
    args = p.parse_args(argv)
    if args.input_dir is None:
        raise ValueError('Input directory (-i) is required.')
    if args.output_dir is None:
        raise ValueError('Output directory (-o) is required.')
    if args.delta_input_dir is None:
        raise ValueError('Delta input directory (-d) is required.')
    if args.debug_mode is not None and args.debug_mode not in ['interpolate_time', 'interpolate_full']:
        raise ValueError('Invalid input for argument --debug_mode! Valid arguments are: "interpolate_time" or "interpolate_full"')
    handed = {k: v for k, v in (('PGW_DELTA_GRID', args.delta_grid), ('PGW_ROTATE_WINDS', args.rotate_winds)) if v is not None}
    found = {k: os.environ.get(k) for k in handed}
    os.environ.update(handed)                                   # the ranks of -p N are new processes: they inherit them
    try:
        return _run_cli(args)
    finally:                                                    # a caller of _cli in a longer-lived process finds what it had
        for k, v in found.items():
            os.environ.pop(k)
            if v is not None:
                os.environ[k] = v


def _source_points_preflight(delta_input_dir, era_paths):
    """What a `--delta_grid source_points` run can object to, from headers and coordinates alone, before a directory is made or a
    rank started: --rotate_winds on a mesh file (every file that exists is asked for its layout), and on the first file that
    exists the pole, the ua / va pair of a rotating run (check_source_wind_files) and the reference's extent errors of every
    source grid (functions.regrid_tables).  ValueError; no field is read, nothing is launched."""
    from . import functions as F, ncio
    paths = [p for p in era_paths if os.path.exists(p)]
    if rotate_winds_request() is not None:
        for p in paths:
            if is_mesh(file_layout(p)):
                _rotation_pole(None, file_layout(p))
    if not paths:
        return
    era5 = _open_era5_target(paths[0])
    targ_lat, targ_lon, H = _point_targets(era5)
    pole = _rotation_pole(era5, H)
    readers = {}
    try:
        for var in DeltaSet.VARS_3D:
            path = os.path.join(delta_input_dir, S.file_name_bases['SCEN-HIST'].format(var))
            if os.path.exists(path):
                readers[var] = ncio.RecordReader(path, var)
        if pole is not None and 'ua' in readers and 'va' in readers:
            check_source_wind_files(readers['ua'], readers['va'])
        seen = set()
        for r in readers.values():
            if S.LAT_GCM in r.coords and S.LON_GCM in r.coords:
                lat, lon = (np.asarray(r.coords[c], dtype=np.float64) for c in (S.LAT_GCM, S.LON_GCM))
                if (lat.tobytes(), lon.tobytes()) not in seen:
                    seen.add((lat.tobytes(), lon.tobytes()))
                    F.regrid_tables(lat, lon, targ_lat.ravel(), targ_lon.ravel())
    finally:
        for r in readers.values():
            r.close()


def _run_cli(args):
    from pathlib import Path
    from .parallel import IterMP
    mode = delta_grid_mode(bands=args.bands)                    # before a directory is made or a rank started
    first = _dt.datetime.strptime(args.first_era_step, '%Y%m%d%H')
    last = _dt.datetime.strptime(args.last_era_step, '%Y%m%d%H')
    inc = _dt.timedelta(hours=args.hour_inc_step)
    steps = []
    t = first
    while t < last + inc:                                   # np.arange(first, last + inc, inc), step_03:594-596
        steps.append(t)
        t += inc
    fargs = dict(delta_input_dir=args.delta_input_dir, ignore_top_pressure_error=args.ignore_top_pressure_error,
                 debug_mode=args.debug_mode)
    step_args = [dict(inp_era_file_path=os.path.join(args.input_dir, S.era5_file_name_base.format(s)),
                      out_era_file_path=os.path.join(args.output_dir, S.era5_file_name_base.format(s)),
                      era_step_dt=s) for s in steps]
    if args.bands:                                              # from the headers, before a directory is made or a rank works
        for s in step_args:
            if os.path.exists(s['inp_era_file_path']):
                _no_bands_on_points(s['inp_era_file_path'])
    if mode == 'source_points':
        _source_points_preflight(args.delta_input_dir, [s['inp_era_file_path'] for s in step_args])
    Path(args.output_dir).mkdir(parents=True, exist_ok=True)
    if args.bands:
        return _run_banded(fargs, step_args)
    func = pgw_for_era5
    if args.debug_mode is not None:                         # step_03:630-635; functions without `stages`: never pipelined
        from . import step_03_debug
        func = (step_03_debug.debug_interpolate_time if args.debug_mode == 'interpolate_time'
                else step_03_debug.debug_interpolate_full)
    imp = IterMP(njobs=args.n_par, run_async=True)
    imp.run(func, fargs, step_args)
    return imp.output


def _run_banded(fargs, step_args):
    """`--bands`: all ranks of the torch.distributed.run launch work on ONE file at a time, in latitude bands."""
    from .parallel import band_max_hook, dist_env, bind_rank_to_numa
    rank, world = dist_env()
    if fargs.get('debug_mode') is not None:
        raise NotImplementedError('debug_mode is a validation aid of the reference and not part of the MI355X hot path')
    if world == 1:
        return [pgw_for_era5(**dict(fargs, **s)) for s in step_args]
    import torch                          # before any HIP call of libpgw_hip.so (see _lib.py)
    import torch.distributed as dist
    created = False
    if not dist.is_initialized():
        backend = os.environ.get('PGW_BANDS_BACKEND') or ('nccl' if torch.cuda.is_available() and torch.cuda.device_count() >= world else 'gloo')
        if backend == 'nccl':
            torch.cuda.set_device(int(os.environ.get('LOCAL_RANK', '0')))
        dist.init_process_group(backend)
        created = True
    bind_rank_to_numa()
    hook = band_max_hook()
    out, err = [], None
    try:
        for s in step_args:
            out.append(pgw_for_era5_banded(s['inp_era_file_path'], s['out_era_file_path'], fargs['delta_input_dir'], s['era_step_dt'],
                                           fargs['ignore_top_pressure_error'], rank, world, hook, dist.barrier))
    except Exception as e:                # noqa: BLE001 - a data error reached every band through the reduce: all ranks are here
        err = e
    if created:
        try:
            dist.destroy_process_group()
        except Exception:                 # noqa: BLE001
            pass
    if err is not None:
        raise err
    return out


if __name__ == '__main__':
    _cli()
