"""The file plan of process_file_device (settings.file_plan, `pgw_step03_file_at`): the library brackets the delta records for the
instant and fills the instant's part of `pgw_file_args` itself, from a plan kept on the Context.  It changes who fills the
struct, never what is in it: with the plan on and off (`PGW_FILE_PLAN=0`) on the same device arrays every output has the same
bits, the filled struct is the one Python builds field by field, a changed setting or another `out` dict never meets a stale
plan, calls the plan does not cover take the host-built struct, and an error comes back with the same code and text.

All cases: 5 x 29 columns (145: two full waves and a partial one, no multiple of 64 or 128), 40 levels."""
import datetime as dt

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

STORAGE = {'f64': (np.float64, False), 'f32ref': (np.float32, True), 'f32fast': (np.float32, False)}
# the synthetic deltas are stamped on the 15th at 12:00: six consecutive hourly instants across that record, and the record
STAMPS = [dt.datetime(2006, 3, 15, 8, 30) + dt.timedelta(hours=i) for i in range(6)] + [dt.datetime(2006, 3, 15, 12)]
OUTPUTS = ('PS', 'T', 'QV', 'U', 'V', 'T_SKIN', 'T_SO', 'FR_SEA_ICE')
OTHER_AXIS = np.array(['1995-%02d-01T00:00:00' % m for m in range(1, 13)], dtype='datetime64[s]')


class _Setup:
    """One synthetic file and its deltas on the device, and counters on the two C entries (pgw_step03_file_at calls
    pgw_step03_file inside the library, which the Python-side counter does not see: the counters tell the host paths apart)."""

    def __init__(self, monkeypatch, storage='f64', seed=5, times_by_var=None, resident=None, deltas=None):
        from pgw4era5_amd import step_03_apply_to_era as s3, synthetic
        from pgw4era5_amd.device import default_context
        self.s3, self.mp = s3, monkeypatch
        self.dtype, self.ref = STORAGE[storage]
        self.case = c = synthetic.make_case(5, 29, 40, seed=seed, dtype=self.dtype)
        self.ctx = ctx = default_context()
        ctx._file_plans.clear()                             # the context is the suite's: start from no plan
        self.deltas = s3.DeltaSet(ctx, deltas or c['deltas'], c['delta_times'], c['plev'], self.dtype, times_by_var=times_by_var,
                                  resident=resident)
        self.era = s3._upload_era(ctx, c['era'], self.dtype)
        self.coeffs = dict(ak=c['era']['ak'], bk=c['era']['bk'], soil1=c['era']['soil1'])
        self.calls = {'pgw_step03_file': 0, 'pgw_step03_file_at': 0}
        for name in self.calls:
            monkeypatch.setattr(ctx.lib, name, self._counted(name, getattr(ctx.lib, name)))

    def _counted(self, name, real):
        def call(*a):
            self.calls[name] += 1
            return real(*a)
        return call

    def run(self, stamp, plan, out, **kw):
        """One file; returns (outputs on the host, info, copy of the pgw_file_args the call was made with, C entry used)."""
        from pgw4era5_amd import _lib
        self.mp.setenv('PGW_FILE_PLAN', '1' if plan else '0')
        before = dict(self.calls)
        self.ctx.set_option('loop_guess', 6)                # every file leaves its own pass count there: same start for both paths
        o, info = self.s3.process_file_device(self.ctx, self.era, self.coeffs, self.deltas, stamp, True, out=out,
                                              ref_dtype=self.ref, **kw)
        assert o is out
        used = [k for k in self.calls if self.calls[k] != before[k]]
        assert len(used) == 1
        res = {k: out[k].numpy() for k in OUTPUTS}
        return res, info, _lib.FileArgs.from_buffer_copy(self.ctx._last_file_args), used[0]


def _same_outputs(a, b, what=''):
    (ra, ia, _, _), (rb, ib, _, _) = a, b
    assert ia['n_iter'] == ib['n_iter'] and ia['max_err'] == ib['max_err'], what
    assert ia['levels_touched'] == ib['levels_touched'] and ia['passes_launched'] == ib['passes_launched'], what
    for k in OUTPUTS:
        assert ra[k].dtype == rb[k].dtype
        assert np.array_equal(ra[k], rb[k], equal_nan=True), '%s %s' % (k, what)


def _same_struct(got, want, what=''):
    """Field by field; soil_depth is a host table each path keeps its own copy of: compared by content."""
    from pgw4era5_amd import _lib
    for name, _ in _lib.FileArgs._fields_:
        g, w = getattr(got, name), getattr(want, name)
        if name == 'soil_depth':
            assert [g[i] for i in range(got.nsoil)] == [w[i] for i in range(want.nsoil)], what
        elif name == 'plev':
            assert [g[i] for i in range(got.nplev)] == [w[i] for i in range(want.nplev)], what
        elif name == 'max_err_hist':
            assert bytes(g) == bytes(w), what                   # as bits: the entries past n_iter are NaN
        else:
            assert g == w, '%s %s: %r != %r' % (name, what, g, w)


@pytest.mark.parametrize('storage', sorted(STORAGE))
def test_same_bits_and_same_struct_with_the_plan_on_and_off(monkeypatch, storage):
    s = _Setup(monkeypatch, storage)
    out = {}
    x_his = set()
    for stamp in STAMPS:
        a = s.run(stamp, True, out)
        b = s.run(stamp, False, out)
        assert (a[3], b[3]) == ('pgw_step03_file_at', 'pgw_step03_file')
        _same_outputs(a, b, str(stamp))
        _same_struct(a[2], b[2], str(stamp))
        assert a[2].ta_b and a[2].PS_out and a[2].per_var_time == 1 and a[2].ref_dtype == int(s.ref)
        x_his.add((a[2].ta_b, a[2].x_hi))
    assert len({p for p, _ in x_his}) == 2                  # the stamps cross a record: two different 'before' records
    assert 0.0 in {x for _, x in x_his}                     # and one of them is a record
    assert len(s.ctx._file_plans) >= 1


def test_plan_is_reused_and_separate_out_dicts_keep_their_own(monkeypatch):
    s = _Setup(monkeypatch)
    out1, out2 = {}, {}
    a1 = s.run(STAMPS[0], True, out1)
    n = len(s.ctx._file_plans)
    s.run(STAMPS[1], True, out1)
    a1 = s.run(STAMPS[0], True, out1)
    assert len(s.ctx._file_plans) == n                     # same arguments, other instants: the same plan
    a2 = s.run(STAMPS[4], True, out2)                       # another out dict: its own buffers, its own plan
    assert len(s.ctx._file_plans) == n + 1
    assert a2[2].T_out != a1[2].T_out and a2[2].PS_out == out2['PS'].ptr
    ref = {}
    _same_outputs(a2, s.run(STAMPS[4], False, ref), 'second out dict')
    still = {k: out1[k].numpy() for k in OUTPUTS}           # the first dict's arrays were not written again
    for k in OUTPUTS:
        assert np.array_equal(still[k], a1[0][k], equal_nan=True), k
    _same_outputs(a1, s.run(STAMPS[0], False, ref), 'first out dict')


def test_changed_settings_never_meet_a_stale_plan(monkeypatch):
    from pgw4era5_amd import settings as S
    s = _Setup(monkeypatch)
    out = {}
    a = s.run(STAMPS[2], True, out)
    assert a[2].thresh == S.thresh_phi_ref_max_error and a[1]['n_iter'] >= 2
    monkeypatch.setattr(S, 'thresh_phi_ref_max_error', 50.0 * a[1]['max_err'][0])   # pass 1 is enough now
    b = s.run(STAMPS[2], True, out)
    c = s.run(STAMPS[2], False, out)
    assert b[3] == 'pgw_step03_file_at' and b[2].thresh == S.thresh_phi_ref_max_error
    assert b[1]['n_iter'] == 1 < a[1]['n_iter']
    _same_outputs(b, c, 'changed threshold')
    _same_struct(b[2], c[2], 'changed threshold')
    monkeypatch.setattr(S, 'adj_factor', 0.8)
    monkeypatch.setattr(S, 'max_n_iter', 25)
    monkeypatch.setattr(S, 'thresh_phi_ref_max_error', 0.15)
    b = s.run(STAMPS[2], True, out, p_ref=50000.0)
    c = s.run(STAMPS[2], False, out, p_ref=50000.0)
    assert (b[2].adj_factor, b[2].max_n_iter, b[2].p_ref) == (0.8, 25, 50000.0)
    _same_outputs(b, c, 'changed adj_factor, max_n_iter, p_ref')
    _same_struct(b[2], c[2], 'changed adj_factor, max_n_iter, p_ref')


@pytest.mark.parametrize('mode', ['local_p_ref', 'i_reinterp'])
def test_template_fields_work_through_the_plan(monkeypatch, mode):
    s = _Setup(monkeypatch)
    kw = dict(p_ref='local') if mode == 'local_p_ref' else dict(i_reinterp=True)
    out = {}
    for stamp in (STAMPS[3], STAMPS[6]):
        a = s.run(stamp, True, out, **kw)
        b = s.run(stamp, False, out, **kw)
        assert a[3] == 'pgw_step03_file_at'
        assert (a[2].local_p_ref, a[2].i_reinterp) == ((1, 0) if mode == 'local_p_ref' else (0, 1))
        _same_outputs(a, b, mode)
        _same_struct(a[2], b[2], mode)


def test_windowed_records_take_the_host_built_struct(monkeypatch):
    s = _Setup(monkeypatch, resident=False)
    r = _Setup(monkeypatch, resident=True)
    assert not s.deltas.dev and r.deltas.dev
    out = {}
    for stamp in (STAMPS[3], STAMPS[4]):
        a = s.run(stamp, True, out)
        assert a[3] == 'pgw_step03_file'
        _same_outputs(a, s.run(stamp, False, {}), 'windowed, plan off')
        b = r.run(stamp, True, {})
        assert b[3] == 'pgw_step03_file_at'
        _same_outputs(a, b, 'windowed against resident')


def test_own_axis_of_tos_and_siconc_goes_through_the_plan(monkeypatch):
    s = _Setup(monkeypatch, times_by_var={'tos': OTHER_AXIS, 'siconc': OTHER_AXIS})
    assert s.deltas.same_axis('tas') and not s.deltas.same_axis('tos')
    out = {}
    for stamp in STAMPS[3:]:
        a = s.run(stamp, True, out)
        b = s.run(stamp, False, out)
        assert a[3] == 'pgw_step03_file_at'
        assert a[2].tos_x_new != a[2].x_new and a[2].siconc_x_new == a[2].tos_x_new and a[2].ts_x_new == a[2].x_new
        _same_outputs(a, b, str(stamp))
        _same_struct(a[2], b[2], str(stamp))


def test_tas_on_another_axis_takes_the_host_built_struct(monkeypatch):
    s = _Setup(monkeypatch, times_by_var={'tas': OTHER_AXIS})
    assert not s.deltas.same_axis('tas')
    out = {}
    for stamp in (STAMPS[3], STAMPS[4]):
        a = s.run(stamp, True, out)
        assert a[3] == 'pgw_step03_file' and a[2].tas_b == a[2].tas_a      # interpolated beforehand on its own axis
        _same_outputs(a, s.run(stamp, False, {}), str(stamp))


def test_keep_hur_and_sub_second_instants_take_the_host_built_struct(monkeypatch):
    s = _Setup(monkeypatch)
    out = {}
    assert s.run(STAMPS[3], True, out, keep_hur=True)[3] == 'pgw_step03_file'
    assert s.run(STAMPS[3].replace(microsecond=250000), True, out)[3] == 'pgw_step03_file'
    assert s.run(STAMPS[3], True, out)[3] == 'pgw_step03_file_at'


def test_error_comes_back_with_the_same_code_and_text(monkeypatch):
    """A column whose historical surface pressure lies above the delta top (functions.py:360-361): status 15, the reference's
    bare ValueError, the column, the library's text - through either path."""
    from pgw4era5_amd import synthetic
    c = synthetic.make_case(5, 29, 40, seed=5)
    bad = {k: v.copy() for k, v in c['deltas'].items()}
    col = 3 * 29 + 17
    bad['ps_hist'].reshape(12, -1)[:, col] = 50.0
    s = _Setup(monkeypatch, deltas=bad)
    out = {}
    seen = []
    for plan in (True, False, True):
        with pytest.raises(ValueError) as e:
            s.run(STAMPS[3], plan, out)
        seen.append((type(e.value), str(e.value), e.value.column, e.value.detail))
    assert s.calls == {'pgw_step03_file_at': 2, 'pgw_step03_file': 1}
    assert seen[0] == seen[1] == seen[2] and seen[0][1:3] == ('', col)
    good = _Setup(monkeypatch)                                      # the context works on after the error
    _same_outputs(good.run(STAMPS[3], True, {}), good.run(STAMPS[3], False, {}))
