"""What every function-level entry of `pgw4era5_amd.functions` hands to the C-ABI, held to a recorded transcript.

Each case calls one entry on small operands under a stand-in context (tests/function_recorder.py, no GPU) and records: the
uploads (shape, dtype, hash), every `pgw_*` call with its scalar arguments and the dtype, shape and hash of the buffer behind
each pointer argument, and the kind, dtype and shape of what came back - or the exception and its text.  The cases cover both
settings of `settings.function_dtype_flow`, float32 / float64 / float32-file / integer operand mixes, ndarray / DeviceArray /
ncio.Field operands (one with its dimensions in another order), absent optional operands and both kinds of p_ref.

The expected transcript, tests/golden/function_call_transcript.json, was recorded from the package as it stood BEFORE the
two dtype flows of each entry were merged into one body: the merged bodies must produce the same calls, argument for
argument and byte for byte.  To record from a checkout of that (or any) commit:

    PYTHONPATH=<checkout> python tests/test_function_call_transcript.py <output.json>
"""
import ctypes as C
import hashlib
import json
import os
import sys
import zlib

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
from function_recorder import RecordingContext                                       # noqa: E402

FIXTURE = os.path.join(HERE, 'golden', 'function_call_transcript.json')

S4, SH, S3, ST = (2, 4, 3, 5), (2, 5, 3, 5), (2, 3, 5), (2, 3, 3, 5)     # fields, half levels, surface, 3 plev levels
D4, D3, D1 = ('time', 'lev', 'lat', 'lon'), ('time', 'lat', 'lon'), ('lev',)
PLEV = [1.0e5, 5.0e4, 1.0e4]
AK, BK = np.array([0.0, 2.0e3, 6.0e3, 3.0e3, 0.0]), np.array([0.0, 0.0, 0.2, 0.7, 1.0])
f4, f8, i4 = np.dtype('float32'), np.dtype('float64'), np.dtype('int32')

# host buffers behind pointer arguments: entry -> {argument index: number of elements, from the arguments}
HOST_LEN = {
    'pgw_replace_delta_sfc': {5: lambda a: a[3]}, 'pgw_replace_delta_sfc_mixed': {7: lambda a: a[5]},
    'pgw_vert_interp_delta': {6: lambda a: a[3]}, 'pgw_vert_interp_delta_mixed': {10: lambda a: a[7]},
    'pgw_regrid_bilinear': dict([(k, lambda a: a[5]) for k in range(8, 13)] + [(k, lambda a: a[6]) for k in range(13, 18)]),
    'pgw_harmonic_smooth': {4: lambda a: 3 * a[2], 5: lambda a: 3 * a[2]},
}


def _arr(kind, a):
    a = np.asarray(a)
    return '%s:%s:%s:%s' % (kind, a.dtype.name, 'x'.join(str(n) for n in a.shape),
                            hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()[:12])


def _kind(r):
    """Type, dtype and shape of a returned value."""
    from pgw4era5_amd.device import DeviceArray
    if r is None or isinstance(r, (bool, int, float, str)):
        return r
    if isinstance(r, (tuple, list)):
        return [_kind(x) for x in r]
    if isinstance(r, dict):
        return {k: _kind(v) for k, v in sorted(r.items())}
    what = '%s:%s:%s' % (type(r).__name__, np.dtype(r.dtype).name, 'x'.join(str(n) for n in r.shape))
    if not isinstance(r, DeviceArray) and hasattr(r, 'dims'):
        what += ':' + ','.join(r.dims)
    return what


class Recorder:
    def __init__(self):
        self.calls, self.uploads = [], []
        self.ctx = RecordingContext(self.observe)

    def _arg(self, name, k, a, args):
        if a is None or isinstance(a, float):
            return a
        if isinstance(a, (int, np.integer)):
            return _arr('dev', self.ctx.mem[a]) if a in self.ctx.mem else int(a)
        if isinstance(a, C._Pointer):
            n = HOST_LEN.get(name, {}).get(k)
            return _arr('host', np.ctypeslib.as_array(a, shape=(int(n(args)),))) if n else 'pointer:' + type(a).__name__
        return type(a).__name__                             # byref(...), a ctypes array of results

    def observe(self, name, args):
        if name == 'to_device':
            self.uploads.append(_arr('up', args[0]))
        elif name == 'set_levels':
            self.calls.append([name] + [None if a is None else _arr('host', a) for a in args])
        else:
            self.calls.append([name] + [self._arg(name, k, a, args) for k, a in enumerate(args)])


def run_case(flow, build):
    """Transcript of one call: `build(F, ctx)` makes the operands (not part of the transcript) and returns the call."""
    from pgw4era5_amd import functions as F, settings
    rec = Recorder()
    old = F.default_context, settings.function_dtype_flow
    F.default_context, settings.function_dtype_flow = (lambda: rec.ctx), flow
    try:
        call = build(F, rec.ctx)
        out = {}
        try:
            out['returns'] = _kind(call())
        except Exception as e:                              # noqa: BLE001 - the exception is what the transcript records
            out['raises'] = [type(e).__name__, str(e)]
    finally:
        F.default_context, settings.function_dtype_flow = old
    return dict(uploads=rec.uploads, calls=rec.calls, **out)


# ------------------------------------------------------------------------------- operands
def _data(name, shape, dtype, lo=1.0, hi=9.0):
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    if np.dtype(dtype).kind == 'i':
        return rng.integers(int(lo), int(hi) + 1, shape).astype(dtype)
    return rng.uniform(lo, hi, shape).astype(dtype)


class Maker:
    """Operands of one case: array kind `kind` (nd, dev, field), dtype mix `mix` (f32, f64, file = float32 fields with
    float64 pressures, int = file with one integer operand)."""

    def __init__(self, ctx, kind, mix):
        self.ctx, self.kind, self.mix = ctx, kind, mix

    def dtype(self, role, int_slot=False):
        if self.mix == 'int' and int_slot:
            return i4
        if self.mix in ('f32', 'f64'):
            return f4 if self.mix == 'f32' else f8
        return f8 if role == 'p' else f4

    def __call__(self, name, shape, role='x', int_slot=False, dims=None, swap=False, coords=None, kind=None):
        from pgw4era5_amd.ncio import Field
        a = _data(name, shape, self.dtype(role, int_slot))
        kind = kind or self.kind
        if kind == 'dev':
            return self.ctx.device_from(a)
        if kind == 'field':
            dims = dims or (D4 if len(shape) == 4 else D3)
            f = Field(a, dims, coords)
            return f.transpose(*reversed(dims)) if swap else f
        return a

    def scalar(self, value, role='x'):
        return np.float32(value) if self.dtype(role) == f4 else float(value)


def _humidity3(entry, first):
    def build(F, ctx, m, variant):
        a, pa, ta = m(first, S4), m('pa', S4, 'p', swap=variant == 'swapped'), m('ta', S4, int_slot=True)
        return lambda: getattr(F, entry)(a, pa, ta)
    return build


def _humidity2(entry, first):
    def build(F, ctx, m, variant):
        a, pa = m(first, S4, int_slot=True), m('pa', S4, 'p', swap=variant == 'swapped')
        return lambda: getattr(F, entry)(a, pa)
    return build


def _svp(entry):
    def build(F, ctx, m, variant):
        pa, ta = m('pa', S4, 'p'), m('ta', S4, int_slot=True)
        if entry.endswith('or_ice'):
            return lambda: getattr(F, entry)(pa, ta, variant != 'ice')
        return lambda: getattr(F, entry)(pa, ta)
    return build


def _integ_geopot(F, ctx, m, variant):
    pa_hl, zgs = m('pa_hl', SH, 'p'), m('zgs', S3, int_slot=True)
    ta, hus = m('ta', S4), m('hus', S4, swap=variant == 'swapped')
    p_ref = m('p_ref', S3, 'p') if variant == 'field' else 3.0e4
    return lambda: F.integ_geopot(pa_hl, zgs, ta, hus, np.arange(1, 6), p_ref, full_column=variant != 'partial')


def _interp_logp_4d(F, ctx, m, variant):
    var, src, trg = m('var', S4, int_slot=True), m('source_P', S4, 'p'), m('targ_P', ST, 'p')
    return lambda: F.interp_logp_4d(var, src, trg, extrapolate=variant)


def _interp_1d(F, ctx, m, variant):
    var, src, trg = m('orig_array', S4, int_slot=True), m('src_p', S4, 'p'), m('targ_p', ST, 'p')
    filled = np.full(ST, -1.0)

    def call():
        r = F.interp_1d_for_timelatlon(var, src, trg, filled, 2, 3, 5, variant)
        return [r, filled]
    return call


def _interp_extrap_1d(F, ctx, m, variant):
    x, y, t = m('src_x', (5,), 'p', dims=D1), m('src_y', (5,), int_slot=True, dims=D1), m('targ_x', (3,), 'p', dims=D1)
    if variant == 'lists':
        x, y, t = x.tolist(), y.tolist(), t.tolist()
    return lambda: F.interp_extrap_1d(x, y, t, 'linear')


def _time_lerp(F, ctx, m, variant):
    b, a = m('v_before', S4), m('v_after', S4, int_slot=True)
    return lambda: F.time_lerp(b, a, 2.0, 0.5)


def _replace_delta_sfc(F, ctx, m, variant):
    P, delta = m('source_P', (5,), 'p', dims=D1), m('delta', (5,), int_slot=True, dims=D1)
    if variant == 'lists':
        P, delta = P.tolist(), delta.tolist()
    return lambda: F.replace_delta_sfc(P, m.scalar(9.5e4), delta, m.scalar(1.5))


def _vert_interp_delta(F, ctx, m, variant):
    coords = {'plev': np.array(PLEV)} if variant == 'coords' else None
    delta, trg = m('delta', ST, dims=('time', 'plev', 'lat', 'lon'), coords=coords), m('target_P', S4, 'p')
    sfc = ps = add = None
    if variant in ('sfc', 'sfc_add', 'coords'):
        sfc, ps = m('delta_sfc', S3, int_slot=True), m('ps_hist', S3)
    if variant == 'sfc_add':
        add = m('add_to', S4)
    if variant == 'add_bcast':
        add = m('add_to', (4, 1, 5), kind='nd')
    return lambda: F.vert_interp_delta(delta, trg, sfc, ps, ignore_top_pressure_error=variant == 'sfc_add',
                                       plev=None if variant == 'coords' else PLEV, add_to=add)


def _integrate_tos(F, ctx, m, variant):
    ops = [m(n, S3, int_slot=n == 'land_frac') for n in ('tos_field', 'ts_field', 'land_frac', 'ice_frac')]
    return lambda: F.integrate_tos(*ops)


def _hybrid_pressure(F, ctx, m, variant):
    ps = m('ps', S3, int_slot=True)
    mid = (None, None) if variant == 'no_mid' else (0.5 * (AK[1:] + AK[:-1]), 0.5 * (BK[1:] + BK[:-1]))
    return lambda: F.hybrid_pressure(AK, BK, ps, *mid)


def _adjust_ps_loop(F, ctx, m, variant):
    PS, FIS, dzg = m('PS', S3), m('FIS', S3, int_slot=True), m('dzg_pref', S3)
    T, QV, ta, hur = m('T', S4), m('QV', S4), m('ta_pgw', S4), m('hur_pgw', S4)
    if variant == 'defaults':
        return lambda: F.adjust_ps_loop(AK, BK, PS, FIS, T, QV, ta, hur, dzg)
    return lambda: F.adjust_ps_loop(AK, BK, PS, FIS, T, QV, ta, hur, dzg, p_ref=3.0e4, adj_factor=0.9, thresh=0.1, max_n_iter=5,
                                    want_hus=False)


def _regrid_field(F, ctx, m, variant):
    field = m('field', S4, int_slot=True)
    return lambda: F.regrid_field(field, [-10.0, 0.0, 10.0], [0.0, 10.0, 20.0, 30.0, 40.0], [-5.0, 5.0], [5.0, 15.0, 25.0])


def _smooth_annual_cycle(F, ctx, m, variant):
    diff = m('diff', S4 if variant == '4d' else (8, 3, 5), dims=D4 if variant == '4d' else D3)
    return lambda: F.smooth_annual_cycle(diff)


ALL_KINDS = [('nd', 'f32'), ('nd', 'f64'), ('nd', 'file'), ('nd', 'int'), ('dev', 'f64'), ('dev', 'file'),
             ('field', 'f64'), ('field', 'file'), ('field', 'int')]
HOST_KINDS = [k for k in ALL_KINDS if k[0] == 'nd']
FEW_KINDS = [('nd', 'file'), ('dev', 'file'), ('field', 'file')]
NO_LEN_KINDS = [('dev', 'file'), ('field', 'file')]     # the two single-column entries take len() of their operands: a TypeError
BOTH = ('common', 'reference')

# entry -> (builder, flows, {variant: (array kind, dtype mix) pairs})
ENTRIES = {
    'specific_to_relative_humidity': (_humidity3('specific_to_relative_humidity', 'hus'), BOTH,
                                      {'plain': ALL_KINDS, 'swapped': [('field', 'file')]}),
    'relative_to_specific_humidity': (_humidity3('relative_to_specific_humidity', 'hur'), BOTH,
                                      {'plain': ALL_KINDS, 'swapped': [('field', 'file')]}),
    'specific_humidity_to_vapor_pressure': (_humidity2('specific_humidity_to_vapor_pressure', 'hus'), BOTH,
                                            {'plain': ALL_KINDS, 'swapped': [('field', 'file')]}),
    'vapor_pressure_to_specific_humidity': (_humidity2('vapor_pressure_to_specific_humidity', 'vapp'), BOTH, {'plain': ALL_KINDS}),
    'saturation_vapor_pressure_water_or_ice': (_svp('saturation_vapor_pressure_water_or_ice'), BOTH,
                                               {'water': ALL_KINDS, 'ice': FEW_KINDS}),
    'saturation_vapor_pressure_water_and_ice': (_svp('saturation_vapor_pressure_water_and_ice'), BOTH, {'plain': ALL_KINDS}),
    'integ_geopot': (_integ_geopot, BOTH, {'scalar': ALL_KINDS, 'field': ALL_KINDS, 'partial': FEW_KINDS, 'swapped': [('field', 'file')]}),
    'interp_logp_4d': (_interp_logp_4d, BOTH, {'off': ALL_KINDS, 'constant': FEW_KINDS}),
    'interp_1d_for_timelatlon': (_interp_1d, BOTH, {'linear': ALL_KINDS, 'nan': FEW_KINDS}),
    'interp_extrap_1d': (_interp_extrap_1d, BOTH, {'arrays': HOST_KINDS + NO_LEN_KINDS, 'lists': [('nd', 'f64'), ('nd', 'int')]}),
    'time_lerp': (_time_lerp, BOTH, {'plain': ALL_KINDS}),
    'replace_delta_sfc': (_replace_delta_sfc, BOTH, {'arrays': HOST_KINDS + NO_LEN_KINDS, 'lists': [('nd', 'f64'), ('nd', 'int')]}),
    'vert_interp_delta': (_vert_interp_delta, BOTH, {'bare': ALL_KINDS, 'sfc': ALL_KINDS, 'sfc_add': ALL_KINDS, 'add_bcast': FEW_KINDS,
                                                     'coords': [('field', 'file'), ('field', 'f64')]}),
    'integrate_tos': (_integrate_tos, BOTH, {'plain': ALL_KINDS}),
    'hybrid_pressure': (_hybrid_pressure, ('common',), {'mid': ALL_KINDS, 'no_mid': FEW_KINDS}),
    'adjust_ps_loop': (_adjust_ps_loop, ('common',), {'explicit': ALL_KINDS, 'defaults': FEW_KINDS}),
    'regrid_field': (_regrid_field, ('common',), {'plain': ALL_KINDS}),
    'smooth_annual_cycle': (_smooth_annual_cycle, ('common',), {'4d': ALL_KINDS, '3d': FEW_KINDS}),
}


def _special_cases():
    """Cases outside the matrix: operands of different kinds in one call, shapes and arguments that must raise before
    anything is uploaded, and a setting that is neither flow."""
    def mixed_kinds(F, ctx):
        hus, pa, ta = _data('hus', S4, f8), ctx.device_from(_data('pa', S4, f4)), _data('ta', S4, f4)
        return lambda: F.specific_to_relative_humidity(hus, pa, ta)

    def broadcast(F, ctx):
        return lambda: F.relative_to_specific_humidity(_data('hur', S4, f4), _data('pa', (4, 1, 1), f8), _data('ta', (1, 1, 3, 5), f4))

    def short_ta(F, ctx):
        return lambda: F.specific_to_relative_humidity(_data('hus', S4, f8), _data('pa', S4, f8), _data('ta', (2, 4, 3, 4), f8))

    def short_device_pa(F, ctx):
        pa = ctx.device_from(_data('pa', (1, 4, 3, 5), f8))
        return lambda: F.specific_humidity_to_vapor_pressure(_data('hus', S4, f8), pa)

    def levels(F, ctx):
        return lambda: F.integ_geopot(_data('pa_hl', SH, f8), _data('zgs', S3, f8), _data('ta', S4, f8), _data('hus', S4, f8),
                                      np.arange(1, 5), 3.0e4)

    def times(F, ctx):
        return lambda: F.interp_logp_4d(_data('var', S4, f8), _data('source_P', (3, 4, 3, 5), f8), _data('targ_P', ST, f8))

    def lone_sfc(F, ctx):
        return lambda: F.vert_interp_delta(_data('delta', ST, f8), _data('target_P', S4, f8), _data('delta_sfc', S3, f8), None, plev=PLEV)

    def no_plev(F, ctx):
        return lambda: F.vert_interp_delta(_data('delta', ST, f8), _data('target_P', S4, f8))

    def short_add_to(F, ctx):
        return lambda: F.vert_interp_delta(_data('delta', ST, f8), _data('target_P', S4, f8), plev=PLEV, add_to=_data('add_to', ST, f8))

    def short_after(F, ctx):
        return lambda: F.time_lerp(_data('v_before', S4, f4), _data('v_after', (2, 4, 3, 4), f4), 2.0, 1.0)

    def bad_mode(entry):
        def build(F, ctx):
            a = _data('a', S4, f8)
            if entry == 'interp_logp_4d':
                return lambda: F.interp_logp_4d(a, a, a, extrapolate='quadratic')
            if entry == 'interp_1d_for_timelatlon':
                return lambda: F.interp_1d_for_timelatlon(a, a, a, np.zeros(S4), 2, 3, 5, 'quadratic')
            return lambda: F.interp_extrap_1d(a[0, :, 0, 0], a[0, :, 0, 0], a[0, :, 0, 0], 'quadratic')
        return build

    def status(rc, entry):
        def build(F, ctx):
            ctx.status = {'pgw_interp_logp_4d': rc, 'pgw_interp_logp_4d_mixed': rc}
            x, y = _data('src_x', (5,), f8), _data('src_y', (5,), f4)
            if entry == 'interp_extrap_1d':                   # masks the two "not ascending" statuses, and only those
                return lambda: F.interp_extrap_1d(x, y, x[:3], 'linear')
            a = _data('a', S4, f8)
            return lambda: F.interp_1d_for_timelatlon(a, a, a, np.zeros(S4), 2, 3, 5, 'linear')
        return build

    special = dict(mixed_kinds=mixed_kinds, broadcast=broadcast, short_ta=short_ta, short_device_pa=short_device_pa, levels=levels,
                   times=times, lone_sfc=lone_sfc, no_plev=no_plev, short_add_to=short_add_to, short_after=short_after)
    for entry in ('interp_logp_4d', 'interp_1d_for_timelatlon', 'interp_extrap_1d'):
        special['bad_mode_' + entry] = bad_mode(entry)
    for rc in (10, 11, 12):
        special['status_%d_interp_extrap_1d' % rc] = status(rc, 'interp_extrap_1d')
    special['status_10_interp_1d_for_timelatlon'] = status(10, 'interp_1d_for_timelatlon')
    for name, build in special.items():
        for flow in BOTH:
            yield 'special/%s/%s' % (name, flow), flow, build
    for entry, (build, _, variants) in ENTRIES.items():       # entries without a reference flow never read the setting
        variant = next(iter(variants))
        yield 'special/bad_setting/%s' % entry, 'fast', (lambda F, ctx, b=build, v=variant: b(F, ctx, Maker(ctx, 'nd', 'f64'), v))


def cases():
    for entry, (build, flows, variants) in ENTRIES.items():
        for variant, kinds in variants.items():
            for kind, mix in kinds:
                for flow in flows:
                    yield ('%s/%s/%s/%s/%s' % (entry, variant, kind, mix, flow), flow,
                           lambda F, ctx, b=build, k=kind, x=mix, v=variant: b(F, ctx, Maker(ctx, k, x), v))
    yield from _special_cases()


def transcript():
    return {name: run_case(flow, build) for name, flow, build in cases()}


def dumps(t):
    return json.dumps(t, sort_keys=True, separators=(',', ':'), indent=None).replace('},"', '},\n"') + '\n'


def test_every_entry_makes_the_recorded_calls():
    with open(FIXTURE) as f:
        want = json.load(f)
    got = json.loads(dumps(transcript()))
    assert sorted(got) == sorted(want)
    differ = [name for name in want if got[name] != want[name]]
    assert not differ, '%d of %d cases differ, the first: %s\n got  %s\n want %s' % (
        len(differ), len(want), differ[0], got[differ[0]], want[differ[0]])


def test_the_matrix_covers_both_flows_all_kinds_and_absent_operands():
    """The fixture is only as good as its cases: every entry in every flow it has, all three array kinds, and the calls
    that take the absent-operand and field-p_ref routes really take them."""
    with open(FIXTURE) as f:
        want = json.load(f)
    for entry, (_, flows, variants) in ENTRIES.items():
        for flow in flows:
            ran = [c for n, c in want.items() if n.startswith(entry + '/') and n.endswith('/' + flow) and 'returns' in c]
            assert ran and all(c['calls'] for c in ran), (entry, flow)
    bare = want['vert_interp_delta/bare/nd/file/reference']['calls'][-1]
    assert bare[0] == 'pgw_vert_interp_delta_mixed' and bare[2:7] == [0, 0, 0, 1, 0]       # delta, -, -, target_P, -
    assert want['integ_geopot/field/nd/file/reference']['calls'][-1][13:15] == [0.0, 'dev:float64:2x3x5:' + _arr('', _data('p_ref', S3, f8))[-12:]]
    assert want['integ_geopot/scalar/nd/file/reference']['calls'][-1][13:15] == [3.0e4, None]
    assert want['special/mixed_kinds/common']['raises'][0] == 'TypeError'
    assert 'returns' in want['special/mixed_kinds/reference']
    assert want['integ_geopot/scalar/nd/f32/reference']['raises'][0] == 'NotImplementedError'
    assert '`pa_hl`' in want['integ_geopot/scalar/nd/f32/reference']['raises'][1]
    for entry in ('hybrid_pressure', 'adjust_ps_loop', 'regrid_field', 'smooth_annual_cycle'):
        assert 'returns' in want['special/bad_setting/' + entry]
    assert want['special/bad_setting/time_lerp']['raises'][0] == 'ValueError'
    for flow in BOTH:
        assert 'returns' in want['special/status_10_interp_extrap_1d/' + flow] and 'returns' in want['special/status_11_interp_extrap_1d/' + flow]
        assert 'raises' in want['special/status_12_interp_extrap_1d/' + flow] and 'raises' in want['special/status_10_interp_1d_for_timelatlon/' + flow]


if __name__ == '__main__':
    import pgw4era5_amd
    print('recording from', os.path.dirname(pgw4era5_amd.__file__), file=sys.stderr)
    with open(sys.argv[1], 'w') as f:
        f.write(dumps(transcript()))
