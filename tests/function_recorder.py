"""A stand-in for `pgw4era5_amd.device.Context` that needs no GPU: it records every library call and every upload, and keeps
"device" memory as host arrays.  Shared by the CPU tests of the function-level API (test_function_shapes.py,
test_function_call_transcript.py)."""
import ctypes as C

import numpy as np


class RecordingLib:
    """Records every pgw_* call and answers it with status 0 (or `ctx.status[entry]`); the copies move bytes between host
    memory and the stand-in's buffers."""

    def __init__(self, ctx):
        self.ctx = ctx

    def pgw_memcpy_d2h(self, handle, dst, src, nbytes):
        buf = self.ctx.mem[src]
        C.memmove(dst, buf.ctypes.data, nbytes)
        return 0

    def __getattr__(self, name):
        if not name.startswith('pgw_'):
            raise AttributeError(name)

        def call(*args):
            self.ctx.calls.append((name, args))
            if self.ctx.observer is not None:         # host buffers behind pointer arguments live only as long as the call
                self.ctx.observer(name, args)
            return self.ctx.status.get(name, 0)
        return call


class RecordingContext:
    """Device memory is a dict of host arrays keyed by a fake address (16-byte aligned, far above any count or size)."""

    def __init__(self, observer=None):
        self.handle, self._live, self.nlev = 1, 0, 0
        self.lib = RecordingLib(self)
        self.mem, self.calls, self.uploads, self.status = {}, [], [], {}
        self.observer = observer
        self._next = 1 << 40

    def _alloc(self, host):
        from pgw4era5_amd.device import DeviceArray
        p = self._next
        self._next += (host.nbytes + 15) // 16 * 16 + 16
        self.mem[p] = host
        return DeviceArray(self, host.shape, host.dtype, ptr=p, owner=self)

    def _check(self, rc):
        assert rc == 0

    def sync(self):
        pass

    def empty(self, shape, dtype):
        return self._alloc(np.zeros(shape, dtype))

    def level_array(self, shape, dtype, cls=None):
        return self.empty(shape, dtype)

    def set_levels(self, ak, bk, akm=None, bkm=None):
        self.nlev = len(ak) - 1
        if self.observer is not None:
            self.observer('set_levels', (ak, bk, akm, bkm))

    def to_device(self, host, dtype=None):
        host = np.array(host, dtype=dtype or host.dtype, order='C')
        self.uploads.append(host.shape)
        if self.observer is not None:
            self.observer('to_device', (host,))
        return self._alloc(host)

    def device(self, shape, dtype=np.float64):
        """A DeviceArray operand made by the test itself (not counted as an upload of the call under test)."""
        return self._alloc(np.ones(shape, dtype))

    def device_from(self, host):
        """Like `device`, holding a copy of `host`."""
        return self._alloc(np.array(host, order='C'))

    def entries(self):
        return [n for n, _ in self.calls]
