"""
The array kinds every function-level entry accepts, and how one of them becomes a kernel operand and a result goes back.

  * `numpy.ndarray` (float32/float64)      -> copied to the device, result returned as ndarray
  * `pgw4era5_amd.device.DeviceArray`      -> used in place, result stays on the device
  * labelled arrays (`pgw4era5_amd.ncio.Field`, or any object with `.values`, `.dims`,
    `.coords`)                             -> like ndarray, result re-wrapped with the labels

`functions.py` and `step_01_extract_deltas.py` build on these; nothing here launches a kernel.
"""
import numpy as np

from . import _lib
from .device import DeviceArray

F32, F64 = np.dtype('float32'), np.dtype('float64')


def is_labelled(x):
    # DeviceArray first: its `.values` is a property that copies the array to the host, and hasattr would evaluate it
    return not isinstance(x, DeviceArray) and hasattr(x, 'values') and hasattr(x, 'dims')


def raw(x):
    """ndarray / DeviceArray behind any accepted input."""
    if isinstance(x, DeviceArray):
        return x
    if is_labelled(x):
        return np.asarray(x.values)
    return np.asarray(x)


def float_dtype(dt):
    """float32 / float64 as they are; anything else (integers, bool) as the float64 numpy's promotion with a python float
    gives."""
    dt = np.dtype(dt)
    return dt if dt in (F32, F64) else F64


def own(x):
    """ndarray (float32 / float64 as it is, anything else as float64) or DeviceArray behind an operand: no cast."""
    r = raw(x)
    if isinstance(r, DeviceArray):
        return r
    return r if r.dtype in (F32, F64) else r.astype(F64)


def common_dtype(*xs):
    """The one dtype of a call in the common flow: float64 as soon as one operand is float64 or integer."""
    for x in xs:
        if x is None:
            continue
        r = raw(x)
        if r.dtype == F64:
            return F64
        if r.dtype != F32 and not isinstance(r, DeviceArray) and r.dtype.kind in 'iu':
            return F64
    return F32


def aligned(x, like):
    """A labelled operand whose dimensions are those of `like` in another order is transposed to `like`'s order (xarray
    aligns operands by dimension NAME; the kernels take positions).  Anything else passes through."""
    if x is None or not (is_labelled(x) and is_labelled(like)):
        return x
    dx, dl = tuple(x.dims), tuple(like.dims)
    if dx != dl and sorted(dx) == sorted(dl) and hasattr(x, 'transpose'):
        return x.transpose(*dl)
    return x


def fit(x, shape, name):
    """Operand `x` for a kernel that indexes it as `shape` (the leading operand's): a host array is broadcast to it like the
    reference's numpy arithmetic would (ValueError when it cannot be), a DeviceArray must have exactly that shape.  Called
    before anything is uploaded or launched: a shorter operand would otherwise be read past its end."""
    shape = tuple(int(n) for n in shape)
    r = raw(x)
    if isinstance(r, DeviceArray):
        if r.shape != shape:
            raise ValueError('%s: device array of shape %s, expected %s' % (name, r.shape, shape))
        return r
    try:
        return np.broadcast_to(r, shape)
    except ValueError:
        raise ValueError('%s: shape %s does not broadcast to %s' % (name, r.shape, shape)) from None


def shape4(x):
    s = raw(x).shape
    if len(s) != 4:
        raise ValueError('expected a 4-D (time, level, lat, lon) array, got shape %s' % (s,))
    return s


def check_extrapolate(extrapolate):
    if extrapolate not in _lib.EXTRAP:
        raise ValueError('Invalid input value for "extrapolate"')
    return _lib.EXTRAP[extrapolate]


def _placed(ctx, r, dtype, shape):
    """DeviceArray `r` viewed as `shape`, or host array `r` uploaded in `dtype` as `shape`."""
    if isinstance(r, DeviceArray):
        return r if shape is None else r.view(shape)
    a = np.ascontiguousarray(r, dtype=dtype)
    if shape is not None:
        a = a.reshape(shape)
    return ctx.to_device(a, a.dtype)


def dev(ctx, x, dtype, shape=None):
    """Device array of `x` in `dtype` (no copy if it already is one of that dtype)."""
    if x is None:
        return None
    r = raw(x)
    if isinstance(r, DeviceArray) and r.dtype != dtype:
        raise TypeError('device arrays of mixed dtype: got %s, expected %s' % (r.dtype, dtype))
    return _placed(ctx, r, dtype, shape)


def dev_own(ctx, x, shape=None):
    """Device array of `x` in ITS OWN dtype (the 'reference' flow: host arrays are uploaded as they are)."""
    return None if x is None else _placed(ctx, own(x), None, shape)


def out_like(dev, like):
    """Return the DeviceArray `dev` in the kind of `like`: DeviceArray as it is; a labelled array re-wrapped with `like`'s
    dimension names and coordinates - `ncio.Field.like(data)`, or `.copy(data=...)` of an `xarray.DataArray` (and anything
    else that offers it), so that the reference's own next line, e.g. `.transpose(TIME_ERA, LEV_ERA, LAT_ERA, LON_ERA)`
    (step_03_apply_to_era.py:91-94), keeps working; a plain ndarray otherwise."""
    if isinstance(like, DeviceArray):
        return dev
    host = dev.numpy()
    if is_labelled(like):
        if hasattr(like, 'like'):
            return like.like(host)
        if hasattr(like, 'copy') and tuple(getattr(like, 'shape', ())) == host.shape:
            try:
                return like.copy(data=host)
            except TypeError:
                pass
    return host
