"""CPU tests of the operand-shape checks of the functions.py mirror.  The flat and column kernels are sized by one operand
and index every other one as if it had the same shape, so a shorter operand would be read past its end on the device.
A stand-in context (no GPU, tests/function_recorder.py) records every library call and every upload: a bad shape must raise
ValueError before any of them, and a host operand that broadcasts must reach the kernel entry at full size, as numpy's
arithmetic would see it."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from function_recorder import RecordingContext                                       # noqa: E402


@pytest.fixture
def ctx(monkeypatch):
    from pgw4era5_amd import functions
    c = RecordingContext()
    monkeypatch.setattr(functions, 'default_context', lambda: c)
    return c


def _bad_calls(F, ctx):
    """(label, call) pairs whose operands cannot be indexed like the leading operand's shape."""
    s = (2, 4, 3, 5)
    one = np.ones(s)
    ph = np.full((2, 5, 3, 5), 5.0e4)
    zgs = np.zeros((2, 3, 5))
    lv1 = np.arange(1, 6)
    return [
        ('q->rh ta short', lambda: F.specific_to_relative_humidity(one, one, np.ones((2, 4, 3, 4)))),
        ('q->rh ta longer time', lambda: F.specific_to_relative_humidity(one, one, np.ones((3, 4, 3, 5)))),
        ('q->rh pa short', lambda: F.specific_to_relative_humidity(one, np.ones((2, 4, 2, 5)), one)),
        ('q->rh device ta', lambda: F.specific_to_relative_humidity(one, one, ctx.device((2, 4, 3, 4)))),
        ('q->rh device ta broadcastable', lambda: F.specific_to_relative_humidity(one, one, ctx.device((1, 4, 3, 5)))),
        ('q->rh device pa', lambda: F.specific_to_relative_humidity(one, ctx.device((2, 4, 3, 4)), one)),
        ('q->rh device pa flat', lambda: F.specific_to_relative_humidity(one, ctx.device((120,)), one)),
        ('rh->q ta short', lambda: F.relative_to_specific_humidity(one, one, np.ones((2, 4, 3, 4)))),
        ('rh->q device ta', lambda: F.relative_to_specific_humidity(one, one, ctx.device((1, 4, 3, 5)))),
        ('rh->q device pa', lambda: F.relative_to_specific_humidity(one, ctx.device((2, 3, 3, 5)), one)),
        ('q->e device pa', lambda: F.specific_humidity_to_vapor_pressure(one, ctx.device((2, 4, 3, 4)))),
        ('q->e pa short', lambda: F.specific_humidity_to_vapor_pressure(one, np.ones((4, 2, 5)))),
        ('e->q device pa', lambda: F.vapor_pressure_to_specific_humidity(one, ctx.device((1, 4, 3, 5)))),
        ('geopot ta time', lambda: F.integ_geopot(ph, zgs, np.ones((3, 4, 3, 5)), np.ones((3, 4, 3, 5)), lv1, 3.0e4)),
        ('geopot ta lat', lambda: F.integ_geopot(ph, zgs, np.ones((2, 4, 2, 5)), np.ones((2, 4, 2, 5)), lv1, 3.0e4)),
        ('geopot ta lon', lambda: F.integ_geopot(ph, zgs, np.ones((2, 4, 3, 4)), np.ones((2, 4, 3, 4)), lv1, 3.0e4)),
        ('geopot device ta', lambda: F.integ_geopot(ph, zgs, ctx.device((1, 4, 3, 5)), ctx.device((1, 4, 3, 5)), lv1, 3.0e4)),
        ('lerp after short', lambda: F.time_lerp(one, np.ones((2, 4, 3, 4)), 2.0, 1.0)),
        ('lerp after longer', lambda: F.time_lerp(one, np.ones((3, 4, 3, 5)), 2.0, 1.0)),
        ('lerp device after', lambda: F.time_lerp(one, ctx.device((2, 4, 3, 4)), 2.0, 1.0)),
        ('vert add_to short', lambda: F.vert_interp_delta(np.ones((2, 3, 3, 5)), one, plev=[1.0e5, 5.0e4, 1.0e4],
                                                           add_to=np.ones((2, 3, 3, 5)))),
        ('vert device add_to', lambda: F.vert_interp_delta(np.ones((2, 3, 3, 5)), one, plev=[1.0e5, 5.0e4, 1.0e4],
                                                            add_to=ctx.device((2, 4, 3, 4)))),
    ]


def test_bad_operand_shapes_raise_before_any_upload_or_launch(ctx):
    from pgw4era5_amd import functions as F
    for label, call in _bad_calls(F, ctx):
        ctx.calls.clear()
        ctx.uploads.clear()
        with pytest.raises(ValueError):
            call()
        assert ctx.calls == [] and ctx.uploads == [], (label, ctx.entries(), ctx.uploads)


def _operand(ctx, name, k):
    """The device buffer behind pointer argument k of the last call of entry `name`."""
    args = [a for n, a in ctx.calls if n == name][-1]
    return ctx.mem[args[k]]


@pytest.mark.parametrize('entry', ['specific_to_relative_humidity', 'relative_to_specific_humidity'])
def test_broadcast_host_operands_reach_the_kernel_at_full_size(ctx, entry):
    from pgw4era5_amd import functions as F
    rng = np.random.default_rng(0)
    x = rng.uniform(size=(2, 4, 3, 5))
    pa = rng.uniform(size=(4, 1, 1))                 # one pressure per level
    ta = rng.uniform(size=(1, 1, 3, 5))              # one temperature per column
    out = getattr(F, entry)(x, pa, ta)
    assert out.shape == x.shape
    assert ctx.entries() == ['pgw_' + entry]
    n, px, pp, pt, po = ctx.calls[-1][1][2:]
    assert n == x.size
    np.testing.assert_array_equal(ctx.mem[px], x)
    np.testing.assert_array_equal(ctx.mem[pp], np.broadcast_to(pa, x.shape))
    np.testing.assert_array_equal(ctx.mem[pt], np.broadcast_to(ta, x.shape))
    assert ctx.mem[po].shape == x.shape


def test_broadcast_host_operands_of_the_other_entries(ctx):
    from pgw4era5_amd import functions as F
    rng = np.random.default_rng(1)
    q = rng.uniform(size=(2, 4, 3, 5))
    pa = rng.uniform(size=(3, 5))
    F.specific_humidity_to_vapor_pressure(q, pa)
    np.testing.assert_array_equal(_operand(ctx, 'pgw_humidity_leaf', 5), np.broadcast_to(pa, q.shape))
    after = rng.uniform(size=(4, 3, 1))
    F.time_lerp(q, after, 2.0, 1.0)
    np.testing.assert_array_equal(_operand(ctx, 'pgw_time_lerp', 4), np.broadcast_to(after, q.shape))
    # integ_geopot: a ta / hus of one time step for a pa_hl of two (level dimensions as they must be)
    ph = np.full((2, 5, 3, 5), 5.0e4)
    ta, hus = rng.uniform(size=(1, 4, 3, 5)), rng.uniform(size=(1, 4, 3, 5))
    F.integ_geopot(ph, np.zeros((2, 3, 5)), ta, hus, np.arange(1, 6), 3.0e4)
    assert [a for n, a in ctx.calls if n == 'pgw_integ_geopot'][-1][2:5] == (2, 4, 15)
    np.testing.assert_array_equal(_operand(ctx, 'pgw_integ_geopot', 7), np.broadcast_to(ta, (2, 4, 3, 5)))
    np.testing.assert_array_equal(_operand(ctx, 'pgw_integ_geopot', 8), np.broadcast_to(hus, (2, 4, 3, 5)))
    add = rng.uniform(size=(4, 1, 5))
    F.vert_interp_delta(np.ones((2, 3, 3, 5)), q, plev=[1.0e5, 5.0e4, 1.0e4], add_to=add)
    args = [a for n, a in ctx.calls if n == 'pgw_vert_interp_delta'][-1]
    np.testing.assert_array_equal(ctx.mem[args[18]], np.broadcast_to(add, q.shape))


def test_matching_device_operands_pass(ctx):
    from pgw4era5_amd import functions as F
    s = (2, 4, 3, 5)
    hus, pa, ta = ctx.device(s), ctx.device(s), ctx.device(s)
    out = F.specific_to_relative_humidity(hus, pa, ta)
    assert out.shape == s and ctx.uploads == []
    assert ctx.calls[-1][1][4:6] == (pa.ptr, ta.ptr)
    out = F.time_lerp(hus, ta, 2.0, 1.0)
    assert ctx.calls[-1][0] == 'pgw_time_lerp' and ctx.calls[-1][1][4] == ta.ptr and ctx.uploads == []
