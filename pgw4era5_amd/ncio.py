"""
Minimal labelled arrays + NetCDF-3 file I/O for the step_02 / step_03 drivers.

The reference does its I/O through xarray (`xr.open_dataset`, `.to_netcdf`; reference
step_03_apply_to_era.py:60,378, functions.py:203, step_02_preproc_deltas.py:127-150).  Neither
xarray nor netCDF4/HDF5 is available to this build, so the drivers use this small layer on
`scipy.io.netcdf_file` (NetCDF-3 classic / 64-bit offset).  It holds only what the hot path's
callers need: named dimensions, coordinate variables, attributes, CF time decoding.
NetCDF-4/HDF5 files must be converted (`nccopy -k cdf5`/`-k 64-bit-offset`) - file formats are
outside the compute path this package replaces (SURVEY.md section 8 f, rank 1).
"""
import datetime as _dt
import re

import numpy as np
from scipy.io import netcdf_file


class Field:
    """A named-dimension array: `.values`, `.dims`, `.coords` (dim -> 1-D array), `.attrs`."""

    def __init__(self, values, dims, coords=None, attrs=None, name=None):
        self.values = np.asarray(values)
        self.dims = tuple(dims)
        if self.values.ndim != len(self.dims):
            raise ValueError('dims %s do not match array of shape %s' % (self.dims, self.values.shape))
        self.coords = dict(coords or {})
        self.attrs = dict(attrs or {})
        self.name = name

    @property
    def shape(self):
        return self.values.shape

    @property
    def dtype(self):
        return self.values.dtype

    def like(self, values, dims=None):
        """Same labels, new data (used by the functions.py mirror to re-wrap results)."""
        values = np.asarray(values)
        dims = self.dims if dims is None else tuple(dims)
        return Field(values, dims, {k: v for k, v in self.coords.items() if k in dims}, self.attrs, self.name)

    def transpose(self, *dims):
        order = [self.dims.index(d) for d in dims]
        return Field(np.transpose(self.values, order), dims, self.coords, self.attrs, self.name)

    def isel(self, **idx):
        v = self.values
        dims = list(self.dims)
        coords = dict(self.coords)
        for d, i in idx.items():
            ax = dims.index(d)
            v = np.take(v, i, axis=ax)
            if np.ndim(i) == 0:
                dims.pop(ax)
                coords.pop(d, None)
            elif d in coords:
                coords[d] = np.asarray(coords[d])[i]
        return Field(v, dims, coords, self.attrs, self.name)

    def __getitem__(self, key):
        return self.coords[key]

    def __repr__(self):
        return 'Field(%s, dims=%s, dtype=%s)' % (self.name, dict(zip(self.dims, self.shape)), self.dtype)


class Dataset:
    """Variables (name -> Field), dimension coordinates and global attributes of one file."""

    def __init__(self, variables=None, attrs=None, record_dim=None):
        self.variables = dict(variables or {})
        self.attrs = dict(attrs or {})
        self.record_dim = record_dim          # name of the unlimited dimension of the file (kept by to_netcdf), or None

    def __contains__(self, name):
        return name in self.variables

    def __getitem__(self, name):
        return self.variables[name]

    def __setitem__(self, name, field):
        if not isinstance(field, Field):
            raise TypeError('Dataset values must be Field objects')
        field.name = name
        self.variables[name] = field

    def __delitem__(self, name):
        del self.variables[name]

    def __getattr__(self, name):
        if name == 'record_dim':              # Datasets unpickled / built before the attribute existed
            return None
        try:
            return self.__dict__['variables'][name]
        except KeyError:
            raise AttributeError(name)

    def dims(self):
        out = {}
        for f in self.variables.values():
            for d, n in zip(f.dims, f.shape):
                out.setdefault(d, n)
        return out

    def close(self):
        pass


# ------------------------------------------------------------------------------ CF time
_UNITS = re.compile(r'^\s*(\w+)\s+since\s+(\d{1,4})-(\d{1,2})-(\d{1,2})(?:[ T](\d{1,2}):(\d{1,2})(?::(\d{1,2}(?:\.\d*)?))?)?')
_SECONDS = {'seconds': 1, 'second': 1, 'secs': 1, 's': 1, 'minutes': 60, 'minute': 60, 'hours': 3600, 'hour': 3600,
            'hrs': 3600, 'h': 3600, 'days': 86400, 'day': 86400, 'd': 86400}
_CUM365 = np.array([0, 31, 59, 90, 120, 151, 181, 212, 243, 273, 304, 334, 365])


def decode_cf_time(values, units, calendar='standard'):
    """CF 'X since Y' numbers -> datetime64[s].  Calendars: standard/gregorian/
    proleptic_gregorian, noleap/365_day (dates map to the same month/day in the standard
    calendar, which is what xarray's `to_datetimeindex()` does, functions.py:219-221) and 360_day
    (day 30 of a 28/29-day February is clipped)."""
    m = _UNITS.match(units)
    if not m:
        raise ValueError('cannot parse time units %r' % units)
    unit = m.group(1).lower()
    if unit not in _SECONDS:
        raise ValueError('unsupported time unit %r' % unit)
    y, mo, d = int(m.group(2)), int(m.group(3)), int(m.group(4))
    hh, mi = int(m.group(5) or 0), int(m.group(6) or 0)
    ss = float(m.group(7) or 0)
    secs = np.asarray(values, dtype=np.float64) * _SECONDS[unit]
    cal = (calendar or 'standard').lower()
    if cal in ('standard', 'gregorian', 'proleptic_gregorian'):
        base = np.datetime64('%04d-%02d-%02dT%02d:%02d:%02d' % (y, mo, d, hh, mi, int(ss)), 's')
        return base + np.round(secs).astype('timedelta64[s]')
    out = []
    for s in np.atleast_1d(secs):
        if cal in ('noleap', '365_day'):
            base_days = y * 365 + _CUM365[mo - 1] + (d - 1)
            tot = base_days * 86400.0 + hh * 3600 + mi * 60 + ss + s
            day, rem = divmod(tot, 86400.0)
            yy, doy = divmod(int(day), 365)
            mm = int(np.searchsorted(_CUM365, doy, side='right'))
            dd = doy - _CUM365[mm - 1] + 1
        elif cal == '360_day':
            base_days = y * 360 + (mo - 1) * 30 + (d - 1)
            tot = base_days * 86400.0 + hh * 3600 + mi * 60 + ss + s
            day, rem = divmod(tot, 86400.0)
            yy, doy = divmod(int(day), 360)
            mm, dd = doy // 30 + 1, doy % 30 + 1
            dd = min(dd, 28 if mm == 2 else 30)
        else:
            raise ValueError('unsupported calendar %r' % calendar)
        rem = int(round(rem))
        out.append(np.datetime64('%04d-%02d-%02d' % (yy, mm, dd), 's') + np.timedelta64(rem, 's'))
    return np.array(out, dtype='datetime64[s]').reshape(np.shape(values))


_CUM366 = np.array([0, 31, 60, 91, 121, 152, 182, 213, 244, 274, 305, 335, 366])


def cf_year_month_day(values, units, calendar='standard'):
    """CF 'X since Y' numbers -> integer (year, month, day) arrays IN THE FILE'S OWN CALENDAR (what `cdo ymonmean` /
    `ydaymean` / `selyear` bin by): standard / gregorian / proleptic_gregorian (the proleptic Gregorian calendar of
    numpy), noleap / 365_day, all_leap / 366_day, 360_day.  Nothing is mapped or clipped: 360_day yields Feb 29 and
    Feb 30, all_leap a Feb 29 in every year.  Times are rounded to whole seconds first, like decode_cf_time."""
    m = _UNITS.match(units)
    if not m:
        raise ValueError('cannot parse time units %r' % units)
    unit = m.group(1).lower()
    if unit not in _SECONDS:
        raise ValueError('unsupported time unit %r' % unit)
    y, mo, d = int(m.group(2)), int(m.group(3)), int(m.group(4))
    hh, mi = int(m.group(5) or 0), int(m.group(6) or 0)
    ss = float(m.group(7) or 0)
    vals = np.asarray(values, dtype=np.float64)
    secs = np.round(vals * _SECONDS[unit]).astype(np.int64)
    cal = (calendar or 'standard').lower()
    if cal in ('standard', 'gregorian', 'proleptic_gregorian'):
        t = np.datetime64('%04d-%02d-%02dT%02d:%02d:%02d' % (y, mo, d, hh, mi, int(ss)), 's') + secs.astype('timedelta64[s]')
        t_y, t_m, t_d = t.astype('datetime64[Y]'), t.astype('datetime64[M]'), t.astype('datetime64[D]')
        year = t_y.astype(np.int64) + 1970
        month = (t_m - t_y.astype('datetime64[M]')).astype(np.int64) + 1
        day = (t_d - t_m.astype('datetime64[D]')).astype(np.int64) + 1
        return year, month, day
    base_secs = hh * 3600 + mi * 60 + int(round(ss))
    if cal in ('noleap', '365_day', 'all_leap', '366_day'):
        cum = _CUM365 if cal in ('noleap', '365_day') else _CUM366
        ylen = int(cum[-1])
        days = (y * ylen + int(cum[mo - 1]) + (d - 1)) + (base_secs + secs) // 86400
        year, doy = days // ylen, days % ylen
        month = np.searchsorted(cum, doy, side='right').astype(np.int64)
        day = doy - cum[month - 1] + 1
        return year, month, day
    if cal == '360_day':
        days = (y * 360 + (mo - 1) * 30 + (d - 1)) + (base_secs + secs) // 86400
        year, doy = days // 360, days % 360
        return year, doy // 30 + 1, doy % 30 + 1
    raise ValueError('unsupported calendar %r' % calendar)


# ------------------------------------------------------------------------------ CF mask and scale
def _float_dtype_for(dtype, has_offset):
    """xarray.coding.variables._choose_float_dtype (2022.12): the dtype packed / masked data decode to."""
    if dtype.kind == 'f' and dtype.itemsize <= 4:
        return np.dtype('float32')
    if dtype.kind in 'iu' and dtype.itemsize <= 2 and not has_offset:
        return np.dtype('float32')
    return np.dtype('float64')


def mask_and_scale(values, attrs):
    """What `xr.open_dataset` does by default (the reference reads the delta files that way, functions.py:203):
    `_FillValue` / `missing_value` -> NaN, then `* scale_factor + add_offset`, in xarray's choice of float dtype.
    Returns (values, attrs without the four encoding attributes).  Non-numeric data and variables without any of the
    attributes pass through untouched (float arrays are modified in place)."""
    keys = ('_FillValue', 'missing_value', 'scale_factor', 'add_offset')
    if values.dtype.kind not in 'fiu' or not any(k in attrs for k in keys):
        return values, attrs
    fills = []
    for k in ('_FillValue', 'missing_value'):
        if k in attrs:
            fills += [x for x in np.atleast_1d(np.asarray(attrs[k])).tolist() if not (isinstance(x, float) and x != x)]
    scale, offset = attrs.get('scale_factor'), attrs.get('add_offset')
    out_dt = _float_dtype_for(values.dtype, offset is not None) if (fills or scale is not None or offset is not None) else values.dtype
    mask = None
    for f in fills:
        m = values == np.asarray(f).astype(values.dtype)
        mask = m if mask is None else (mask | m)
    if values.dtype != out_dt:
        values = values.astype(out_dt)
    if mask is not None and mask.any():
        values[mask] = np.nan
    if scale is not None:
        values *= np.asarray(scale).reshape(-1)[0]
    if offset is not None:
        values += np.asarray(offset).reshape(-1)[0]
    return values, {k: v for k, v in attrs.items() if k not in keys}


# ------------------------------------------------------------------------------ file I/O
def _attrs(obj):
    out = {}
    for k, v in obj._attributes.items():
        if isinstance(v, bytes):
            v = v.decode('utf-8', 'replace')
        out[k] = v
    return out


# NetCDF classic header (CDF-1 / CDF-2 / CDF-5), parsed here so that the reader knows every variable's byte
# range and can `pread` it straight into a caller-supplied (pinned) buffer.
_NC_DTYPE = {1: 'i1', 2: 'S1', 3: 'i2', 4: 'i4', 5: 'f4', 6: 'f8', 7: 'u1', 8: 'u2', 9: 'u4', 10: 'i8', 11: 'u8'}
BIG_VARIABLE = 16 << 20                  # bytes; larger variables are read concurrently / kept raw on request


class _Cursor:
    def __init__(self, fd):
        self.fd, self.buf, self.pos = fd, b'', 0

    def take(self, n):
        import os
        while self.pos + n > len(self.buf):
            more = os.pread(self.fd, max(1 << 20, self.pos + n - len(self.buf)), len(self.buf))
            if not more:
                raise ValueError('truncated header')
            self.buf += more
        out = self.buf[self.pos:self.pos + n]
        self.pos += n
        return out

    def i32(self):
        return int.from_bytes(self.take(4), 'big', signed=True)

    def i64(self):
        return int.from_bytes(self.take(8), 'big', signed=True)


def _parse_header(fd, file_size):
    """-> dict(version, numrecs, dims [(name, len)], attrs, vars [dict(name, dims, attrs, dtype, begin, shape,
    record, nbytes)], recsize).  `nbytes` is per record for record variables."""
    c = _Cursor(fd)
    magic = c.take(4)
    if magic[:3] != b'CDF' or magic[3] not in (1, 2, 5):
        raise ValueError('magic %r' % magic)
    version = magic[3]
    nonneg = c.i64 if version == 5 else c.i32

    def name():
        n = nonneg()
        raw = c.take(n)
        c.take(-n % 4)
        return raw.decode('utf-8', 'replace')

    def att_list():
        tag = c.i32()
        n = nonneg()
        if tag == 0:
            return {}
        if tag != 0x0C:
            raise ValueError('attribute list tag %#x' % tag)
        out = {}
        for _ in range(n):
            k = name()
            t = c.i32()
            cnt = nonneg()
            if t not in _NC_DTYPE:
                raise ValueError('attribute type %d' % t)
            dt = np.dtype(_NC_DTYPE[t])
            raw = c.take(cnt * dt.itemsize)
            c.take(-(cnt * dt.itemsize) % 4)
            if t == 2:
                out[k] = raw.rstrip(b'\x00').decode('utf-8', 'replace')
            else:
                v = np.frombuffer(raw, dtype=dt.newbyteorder('>')).astype(dt)
                out[k] = v[0] if v.shape == (1,) else v
        return out

    numrecs = nonneg()
    if version != 5 and numrecs == -1:
        numrecs = None                                           # STREAMING: derived from the file size below
    tag, n = c.i32(), nonneg()
    if tag not in (0, 0x0A):
        raise ValueError('dimension list tag %#x' % tag)
    dims = [(name(), nonneg()) for _ in range(n if tag else 0)]
    gatts = att_list()
    tag, n = c.i32(), nonneg()
    if tag not in (0, 0x0B):
        raise ValueError('variable list tag %#x' % tag)
    variables = []
    for _ in range(n if tag else 0):
        vname = name()
        nd = nonneg()
        dimids = [nonneg() for _ in range(nd)]
        vatts = att_list()
        t = c.i32()
        nonneg()                                                 # vsize: unreliable for > 4 GiB, recomputed
        begin = c.i32() if version == 1 else c.i64()
        if t not in _NC_DTYPE:
            raise ValueError('variable type %d' % t)
        dt = np.dtype(_NC_DTYPE[t])
        record = nd > 0 and dims[dimids[0]][1] == 0
        shape = [dims[i][1] for i in dimids]
        inner = int(np.prod(shape[1:] if record else shape, dtype=np.int64))
        variables.append(dict(name=vname, dims=tuple(dims[i][0] for i in dimids), attrs=vatts, dtype=dt, begin=begin,
                              shape=shape, record=record, nbytes=inner * dt.itemsize))
    recs = [v for v in variables if v['record']]
    if len(recs) == 1:
        recsize = recs[0]['nbytes']                              # a single record variable is not padded
    else:
        recsize = sum(v['nbytes'] + (-v['nbytes'] % 4) for v in recs)
    if recs and numrecs is None:
        numrecs = (file_size - min(v['begin'] for v in recs)) // recsize if recsize else 0
    for v in recs:
        v['shape'][0] = numrecs or 0
    return dict(version=version, numrecs=numrecs or 0, dims=dims, attrs=gatts, vars=variables, recsize=recsize)


def _pread_into(fd, buf, offset):
    """Fill the writable byte buffer from the file (the kernel copies from the page cache straight into `buf`;
    the GIL is released during the call)."""
    import os
    mv = memoryview(buf).cast('B')
    while len(mv):
        n = os.preadv(fd, [mv[:1 << 30]], offset)
        if n <= 0:
            raise IOError('unexpected end of file')
        offset += n
        mv = mv[n:]


def placeholder(shape, dtype):
    """An array of the given shape and dtype that owns one element (all strides 0): stands for a variable whose data are
    read or written elsewhere (band-wise I/O) wherever only shape and dtype matter - the header of to_netcdf's layout."""
    return np.lib.stride_tricks.as_strided(np.zeros(1, dtype=dtype), shape=tuple(int(n) for n in shape),
                                           strides=(0,) * len(shape), writeable=False)


def is_placeholder(a):
    return isinstance(a, np.ndarray) and a.size > 1 and all(st == 0 for st in a.strides)


def open_dataset(path, decode_times=True, threads=4, raw_big=False, alloc=None, decode_mask_scale=None, skip=()):
    """Read a NetCDF-3 file completely into memory (`xr.open_dataset(...).load()`).
    decode_times=False corresponds to the reference's `decode_cf=False` (step_03:60: the ERA5 file is taken raw);
    the default decodes like a plain `xr.open_dataset` (the delta files, functions.py:203): CF times AND
    `_FillValue` / `missing_value` -> NaN, `scale_factor` / `add_offset` applied (`decode_mask_scale`, default = decode_times).

    Every variable is `pread` into its array (large ones concurrently) and converted from the file's big-endian
    layout in place.  With `raw_big=True` variables of at least BIG_VARIABLE bytes are NOT converted: their
    `.values` keep the big-endian dtype of the file ('>f4'), for `DeviceArray.copy_from` to convert on the GPU;
    `alloc(nbytes) -> writable uint8 array` supplies their buffers (pinned host memory in the step_03 driver).
    PGW_NC_READER=scipy selects the previous reader built on scipy.io.netcdf_file.
    skip: names of variables NOT to read - they come back as placeholders of the right shape and dtype (band-wise I/O:
    every rank reads only its latitude rows of the large fields, read_band)."""
    import os
    from concurrent.futures import ThreadPoolExecutor
    if decode_mask_scale is None:
        decode_mask_scale = decode_times
    if os.environ.get('PGW_NC_READER') == 'scipy':
        return _open_dataset_scipy(path, decode_times, threads, decode_mask_scale)
    fd = os.open(path, os.O_RDONLY)
    try:
        try:
            hdr = _parse_header(fd, os.fstat(fd).st_size)
        except (ValueError, IndexError) as e:
            raise IOError('%s is not a NetCDF-3 file (%s). NetCDF-4/HDF5 files must be converted, e.g. '
                          '`nccopy -k 64-bit-offset in.nc out.nc`.' % (path, e))

        def read(v):
            dt = v['dtype']
            nrec = hdr['numrecs'] if v['record'] else 1
            total = v['nbytes'] * nrec
            if v['name'] in skip:                                # data taken elsewhere (read_band): shape and dtype only
                return placeholder(v['shape'], dt)
            big = total >= BIG_VARIABLE
            if big and alloc is not None:
                buf = alloc(total)[:total]
            else:
                buf = np.empty(total, dtype=np.uint8)
            for r in range(nrec):
                if v['nbytes']:
                    _pread_into(fd, buf[r * v['nbytes']:(r + 1) * v['nbytes']], v['begin'] + r * hdr['recsize'])
            arr = buf.view(dt.newbyteorder('>') if dt.itemsize > 1 else dt).reshape(v['shape'])
            if dt.itemsize > 1 and not (big and raw_big):
                arr = arr.byteswap(inplace=True).view(dt)        # one pass, no second array
            return arr

        big = [v for v in hdr['vars'] if v['nbytes'] * (hdr['numrecs'] if v['record'] else 1) >= BIG_VARIABLE]
        data = {}
        if len(big) > 1 and threads > 1:
            with ThreadPoolExecutor(max_workers=min(threads, len(big))) as pool:
                for v, arr in zip(big, pool.map(read, big)):
                    data[v['name']] = arr
        for v in hdr['vars']:
            if v['name'] not in data:
                data[v['name']] = read(v)
    finally:
        os.close(fd)
    rec_dims = [n for n, length in hdr['dims'] if length == 0]
    ds = Dataset(attrs=hdr['attrs'], record_dim=rec_dims[0] if rec_dims else None)
    if decode_mask_scale:
        for v in hdr['vars']:
            if v['name'] not in skip:
                data[v['name']], v['attrs'] = mask_and_scale(data[v['name']], v['attrs'])
    coords = {}
    for v in hdr['vars']:
        if v['dims'] == (v['name'],):
            arr = data[v['name']]
            if decode_times and 'since' in str(v['attrs'].get('units', '')):
                arr = decode_cf_time(arr, v['attrs']['units'], v['attrs'].get('calendar', 'standard'))
                data[v['name']] = arr
            coords[v['name']] = arr
    for v in hdr['vars']:
        ds.variables[v['name']] = Field(data[v['name']], v['dims'], {d: coords[d] for d in v['dims'] if d in coords},
                                        v['attrs'], v['name'])
    return ds


class RecordReader:
    """One variable of a NetCDF-3 file read one record (index along its FIRST dimension) at a time: `pread` of that record's
    bytes, byte order converted, decoded like `open_dataset` (`_FillValue` / `missing_value` -> NaN, scale / offset).  For
    delta files whose records do not all fit on the device - 365 daily records of a 19-level 0.25 deg variable are 144 GB in
    float32 - of which a run needs two at a time (load_delta, functions.py:240-292).  Everything else of the file (the
    coordinates) is read once: `.coords` (times decoded), `.dims`, `.attrs`, `.nrec`, `.rec_shape`, `.dtype` (decoded)."""

    def __init__(self, path, var, decode_times=True):
        import os
        self.path, self.var = path, var
        fd = os.open(path, os.O_RDONLY)
        try:
            try:
                hdr = _parse_header(fd, os.fstat(fd).st_size)
            except (ValueError, IndexError) as e:
                raise IOError('%s is not a NetCDF-3 file (%s).' % (path, e))
            byname = {v['name']: v for v in hdr['vars']}
            if var not in byname:
                raise KeyError(var)
            v = byname[var]
            if len(v['shape']) < 1:
                raise ValueError('%s has no dimension to read records along' % var)
            self._v, self._recsize = v, hdr['recsize']
            self.dims, self.nrec, self.rec_shape = v['dims'], int(v['shape'][0]), tuple(int(n) for n in v['shape'][1:])
            self._inner = int(np.prod(self.rec_shape, dtype=np.int64)) * v['dtype'].itemsize
            self.coords = {}
            for d in self.dims:
                if d in byname and byname[d]['dims'] == (d,):
                    c = byname[d]
                    nrec = hdr['numrecs'] if c['record'] else 1
                    buf = np.empty(c['nbytes'] * nrec, dtype=np.uint8)
                    for r in range(nrec):
                        if c['nbytes']:
                            _pread_into(fd, buf[r * c['nbytes']:(r + 1) * c['nbytes']], c['begin'] + r * hdr['recsize'])
                    arr = buf.view(c['dtype'].newbyteorder('>') if c['dtype'].itemsize > 1 else c['dtype']).reshape(c['shape'])
                    arr = arr.astype(c['dtype'])
                    arr, catt = mask_and_scale(arr, c['attrs'])
                    if decode_times and 'since' in str(catt.get('units', '')):
                        arr = decode_cf_time(arr, catt['units'], catt.get('calendar', 'standard'))
                    self.coords[d] = arr
            probe, self.attrs = mask_and_scale(np.zeros(1, dtype=v['dtype']), dict(v['attrs']))
            self.dtype = probe.dtype
            self.file_dtype, self.file_attrs = v['dtype'], dict(v['attrs'])   # the NetCDF type and the attributes as stored
        finally:
            os.close(fd)
        self._fd = None
        self._lock = __import__('threading').Lock()

    def read_record_raw(self, r, out=None):
        """Record r as the file holds it: the `pread` alone, no byte swap and no decoding.  -> array of `rec_shape` in the
        file's big-endian dtype ('>f4', '>i2', ...; `file_dtype` with the byte order of the file), a view of `out` when a
        writable C-contiguous buffer of the record's size is given."""
        import os
        r = int(r)
        if not 0 <= r < self.nrec:
            raise IndexError(r)
        v = self._v
        with self._lock:
            if self._fd is None:
                self._fd = os.open(self.path, os.O_RDONLY)
        if out is None:
            buf = np.empty(self._inner, dtype=np.uint8)
        else:
            buf = out.reshape(-1).view(np.uint8)
            if buf.size != self._inner or not np.shares_memory(buf, out):
                raise ValueError('out must be a C-contiguous buffer of %d bytes' % self._inner)
        # a record variable's records are `recsize` apart; a fixed-size variable's first dimension is contiguous
        off = v['begin'] + (r * self._recsize if v['record'] else r * self._inner)
        if self._inner:
            _pread_into(self._fd, buf, off)
        return buf.view(v['dtype'].newbyteorder('>') if v['dtype'].itemsize > 1 else v['dtype']).reshape(self.rec_shape)

    def read_record(self, r):
        import os
        r = int(r)
        if not 0 <= r < self.nrec:
            raise IndexError(r)
        v = self._v
        with self._lock:
            if self._fd is None:
                self._fd = os.open(self.path, os.O_RDONLY)
        buf = np.empty(self._inner, dtype=np.uint8)
        # a record variable's records are `recsize` apart; a fixed-size variable's first dimension is contiguous
        off = v['begin'] + (r * self._recsize if v['record'] else r * self._inner)
        if self._inner:
            _pread_into(self._fd, buf, off)
        arr = buf.view(v['dtype'].newbyteorder('>') if v['dtype'].itemsize > 1 else v['dtype']).reshape(self.rec_shape)
        if v['dtype'].itemsize > 1:
            arr = arr.byteswap(inplace=True).view(v['dtype'])
        return mask_and_scale(arr, dict(v['attrs']))[0]

    @property
    def nbytes(self):
        return self.nrec * int(np.prod(self.rec_shape, dtype=np.int64)) * self.dtype.itemsize

    def close(self):
        import os
        with self._lock:
            if self._fd is not None:
                os.close(self._fd)
                self._fd = None

    def __del__(self):
        try:
            self.close()
        except Exception:              # noqa: BLE001
            pass


def _open_dataset_scipy(path, decode_times=True, threads=4, decode_mask_scale=None):
    """The reader of the first version: scipy.io.netcdf_file over a memory map, every variable converted to a
    native-endian copy."""
    from concurrent.futures import ThreadPoolExecutor
    try:
        nc = netcdf_file(path, 'r', mmap=True)
    except (TypeError, ValueError) as e:
        raise IOError('%s is not a NetCDF-3 file (%s). NetCDF-4/HDF5 files must be converted, e.g. '
                      '`nccopy -k 64-bit-offset in.nc out.nc`.' % (path, e))
    try:
        ds = Dataset(attrs=_attrs(nc))
        names = list(nc.variables)

        def convert(name):
            var = nc.variables[name]
            src = var.data
            native = src.dtype.newbyteorder('=') if src.dtype.byteorder in ('>', '<') else src.dtype
            return np.array(src, dtype=native, copy=True, order='C'), tuple(var.dimensions), _attrs(var)

        big = [n for n in names if nc.variables[n].data.nbytes >= BIG_VARIABLE]
        raw = {}
        if len(big) > 1 and threads > 1:
            with ThreadPoolExecutor(max_workers=min(threads, len(big))) as pool:
                for n, r in zip(big, pool.map(convert, big)):
                    raw[n] = r
        for n in names:
            if n not in raw:
                raw[n] = convert(n)
    finally:
        try:
            nc.close()
        except Exception:           # scipy complains if views of the map are still alive; all data were copied
            pass
    if decode_mask_scale or (decode_mask_scale is None and decode_times):
        for name in list(raw):
            data, dims, attrs = raw[name]
            data, attrs = mask_and_scale(data, attrs)
            raw[name] = (data, dims, attrs)
    coords = {}
    for name, (data, dims, attrs) in raw.items():
        if dims == (name,):
            if decode_times and 'since' in str(attrs.get('units', '')):
                data = decode_cf_time(data, attrs['units'], attrs.get('calendar', 'standard'))
            coords[name] = data
    for name in names:
        data, dims, attrs = raw[name]
        if name in coords:
            data = coords[name]
        ds.variables[name] = Field(data, dims, {d: coords[d] for d in dims if d in coords}, attrs, name)
    return ds


_NC_TYPE = {'i1': 1, 'S1': 2, 'i2': 3, 'i4': 4, 'f4': 5, 'f8': 6}


def _pad4(b):
    return b + b'\x00' * (-len(b) % 4)


def _nc_name(name):
    import struct
    raw = name.encode('utf-8')
    return struct.pack('>i', len(raw)) + _pad4(raw)


def _nc_atts(attrs):
    import struct
    if not attrs:
        return b'\x00' * 8                                   # ABSENT
    out = struct.pack('>ii', 0x0C, len(attrs))
    for k, v in attrs.items():
        out += _nc_name(k)
        if isinstance(v, bytes):
            v = v.decode('utf-8', 'replace')
        if isinstance(v, str):
            raw = v.encode('utf-8')
            out += struct.pack('>ii', 2, len(raw)) + _pad4(raw)
        else:
            arr = np.atleast_1d(np.asarray(v))
            if arr.dtype == np.int64:
                arr = arr.astype(np.int32)
            if arr.dtype == np.bool_:
                arr = arr.astype(np.int8)
            key = arr.dtype.str[1:]
            if key not in _NC_TYPE or key == 'S1':
                raw = str(v).encode('utf-8')
                out += struct.pack('>ii', 2, len(raw)) + _pad4(raw)
            else:
                out += struct.pack('>ii', _NC_TYPE[key], arr.size) + _pad4(arr.astype(arr.dtype.newbyteorder('>')).tobytes())
    return out


def _nc_header(attrs, dims, record_dim, numrecs, specs, begins, dim_ids):
    """Bytes of a CDF-2 (64-bit offset) header.  specs: dicts with name, dims, attrs, key (numpy dtype code), vsize."""
    import struct
    h = b'CDF\x02' + struct.pack('>i', numrecs)
    if dims:
        h += struct.pack('>ii', 0x0A, len(dims))
        for d, n in dims.items():
            h += _nc_name(d) + struct.pack('>i', 0 if d == record_dim else n)
    else:
        h += b'\x00' * 8
    h += _nc_atts(attrs)
    if specs:
        h += struct.pack('>ii', 0x0B, len(specs))
        for sp, b in zip(specs, begins):
            h += _nc_name(sp['name']) + struct.pack('>i', len(sp['dims']))
            for d in sp['dims']:
                h += struct.pack('>i', dim_ids[d])
            h += _nc_atts(sp['attrs'])
            # vsize is an UNSIGNED 32-bit field; sizes that do not fit are written as 2^32 - 1 (the CDF-2 convention:
            # readers recompute the size of such variables from their shape - this module's reader always does)
            h += struct.pack('>iI', _NC_TYPE[sp['key']], sp['vsize'] if sp['vsize'] < 2 ** 32 else 0xFFFFFFFF)
            h += struct.pack('>q', b)
    else:
        h += b'\x00' * 8
    return h


def _plan(ds):
    """Layout of a Dataset as a NetCDF-3 64-bit-offset file: (header bytes, specs, begins, total size, recsize, numrecs).
    Only shapes and dtypes are looked at (placeholders do)."""
    dims = {}
    for f in ds.variables.values():
        for d, n in zip(f.dims, f.shape):
            if d in dims and dims[d] != int(n):
                raise ValueError('dimension %s has inconsistent lengths %d and %d' % (d, dims[d], n))
            dims.setdefault(d, int(n))
    dim_ids = {d: i for i, d in enumerate(dims)}
    record_dim = ds.record_dim if ds.record_dim in dims else None
    numrecs = dims[record_dim] if record_dim else 0
    # variables: data converted lazily (dtype decided here)
    specs = []
    for name, f in ds.variables.items():
        data = f.values
        attrs = dict(f.attrs)
        if data.dtype.kind == 'M':
            data = (data.astype('datetime64[s]') - np.datetime64('1970-01-01T00:00:00', 's')).astype(np.float64)
            attrs['units'] = 'seconds since 1970-01-01 00:00:00'
            attrs['calendar'] = 'proleptic_gregorian'
        if data.dtype == np.int64:
            data = data.astype(np.int32)
        if data.dtype == np.bool_:
            data = data.astype(np.int8)
        key = data.dtype.str[1:]
        if key not in _NC_TYPE:             # 'S1': NC_CHAR variables (e.g. the scalar `char rotated_pole` grid-mapping carrier)
            raise TypeError('variable %s: dtype %s cannot be stored in NetCDF-3' % (name, data.dtype))
        record = record_dim is not None and len(f.dims) > 0 and f.dims[0] == record_dim
        nbytes = int(data.size) * data.dtype.itemsize
        per = nbytes // numrecs if (record and numrecs) else (0 if record else nbytes)      # bytes per record / of the variable
        specs.append(dict(name=name, dims=f.dims, data=data, attrs=attrs, key=key, nbytes=nbytes, record=record, per=per,
                          vsize=per + (-per % 4)))
    recs = [sp for sp in specs if sp['record']]
    if len(recs) == 1:
        recs[0]['vsize'] = recs[0]['per']                       # a single record variable is not padded (classic format rule)
    recsize = sum(sp['vsize'] for sp in recs)

    def layout(hlen):
        begins, off = [None] * len(specs), hlen
        for i, sp in enumerate(specs):                           # fixed-size variables first, in header order
            if not sp['record']:
                begins[i] = off
                off += sp['vsize']
        for i, sp in enumerate(specs):                           # then the first record
            if sp['record']:
                begins[i] = off
                off += sp['vsize']
        return begins, off + recsize * max(numrecs - 1, 0)

    hlen = len(_nc_header(ds.attrs, dims, record_dim, numrecs, specs, [0] * len(specs), dim_ids))
    begins, total = layout(hlen)
    hdr = _nc_header(ds.attrs, dims, record_dim, numrecs, specs, begins, dim_ids)
    assert len(hdr) == hlen
    return hdr, specs, begins, total, recsize, numrecs


def to_netcdf(ds, path, threads=None, skip=()):
    """Write a Dataset as NetCDF-3 64-bit-offset (`.to_netcdf(path, mode='w')`, step_03:378).

    Native writer (the classic format is a header + big-endian arrays): every variable is byte-swapped in one pass (not
    at all if it is already big-endian) and written with `os.pwrite` at its offset, large variables in 64 MiB pieces on
    `threads` threads - scipy's writer makes three copies of every array under the GIL and was the bottleneck of the
    whole command line (1.06 s per 2.3 GB file; PGW_NC_WRITER=scipy selects it).
    `ds.record_dim` (set by open_dataset from the input file's unlimited dimension): variables whose first dimension it
    is are written as record variables - dimension length 0 in the header, `numrecs` records interleaved after the
    fixed-size variables - so the ERA5 file keeps its unlimited `time` like the reference's `to_netcdf` does.
    skip: variables whose space is laid out (header, file size) but whose data are NOT written here (placeholders allowed):
    the ranks of a band-wise run write their latitude rows of them (BandedWriter)."""
    import os
    from concurrent.futures import ThreadPoolExecutor
    if os.environ.get('PGW_NC_WRITER') == 'scipy' and not skip:
        return _to_netcdf_scipy(ds, path)
    if threads is None:
        threads = int(os.environ.get('PGW_NC_WRITE_THREADS', '8'))
    hdr, specs, begins, total, recsize, numrecs = _plan(ds)
    fd = os.open(path, os.O_WRONLY | os.O_CREAT | os.O_TRUNC, 0o644)
    try:
        os.ftruncate(fd, total)
        os.pwrite(fd, hdr, 0)
        CH = 64 << 20                                            # swap + write in 64 MiB pieces
        flats = [None if sp['name'] in skip else np.ascontiguousarray(sp['data']).reshape(-1) for sp in specs]

        def write_piece(task):
            i, s0, s1, pos = task
            flat = flats[i]
            # one pass: copy + byte swap; no copy at all if the data are already big-endian (raw I/O path)
            chunk = flat[s0:s1].astype(flat.dtype.newbyteorder('>'), copy=False)
            mv = memoryview(chunk).cast('B')
            while len(mv):
                n = os.pwrite(fd, mv, pos)
                pos += n
                mv = mv[n:]
            # padding bytes are already zero (ftruncate)

        tasks, small = [], []
        for i, sp in enumerate(specs):
            if flats[i] is None:
                continue
            item = flats[i].dtype.itemsize
            if sp['record']:                                     # record r of the variable starts at begin + r * recsize
                n_el = sp['per'] // item
                pieces = [(r * n_el, (r + 1) * n_el, begins[i] + r * recsize) for r in range(numrecs)]
            else:
                pieces = [(0, flats[i].size, begins[i])]
            for e0, e1, pos in pieces:
                if e1 <= e0:
                    continue
                if (e1 - e0) * item >= BIG_VARIABLE:
                    step = max(CH // max(item, 1), 1)
                    tasks += [(i, s0, min(s0 + step, e1), pos + (s0 - e0) * item) for s0 in range(e0, e1, step)]
                else:
                    small.append((i, e0, e1, pos))
        if len(tasks) > 1 and threads > 1:
            with ThreadPoolExecutor(max_workers=min(threads, len(tasks))) as pool:
                list(pool.map(write_piece, tasks))
        else:
            for t in tasks:
                write_piece(t)
        for t in small:
            write_piece(t)
    finally:
        os.close(fd)


# ------------------------------------------------------------------------------ one variable of an existing file
# postproc_cosmo/extpar_adapt.py opens the extpar file in append mode and assigns to one variable; here the variable's byte
# ranges come from the header and nothing else of the file is read or written.
def _variable_ranges(fd, name):
    """-> (header entry of `name`, [(file offset, byte count)] of its data in C order): one range for a fixed-size variable,
    one per record for a record variable.  KeyError when the file has no such variable."""
    import os
    hdr = _parse_header(fd, os.fstat(fd).st_size)
    for v in hdr['vars']:
        if v['name'] == name:
            if v['record']:
                return v, [(v['begin'] + r * hdr['recsize'], v['nbytes']) for r in range(hdr['numrecs'])]
            return v, [(v['begin'], v['nbytes'])]
    raise KeyError(name)


def _file_dtype(v):
    return v['dtype'].newbyteorder('>') if v['dtype'].itemsize > 1 else v['dtype']


def read_variable_raw(path, name):
    """One variable as the file holds it: (array of the variable's shape in the file's big-endian dtype - '>f4', '>i2', ...;
    no byte swap and no decoding -, its dimension names, its attributes as stored).  Nothing else of the file is read."""
    import os
    fd = os.open(path, os.O_RDONLY)
    try:
        v, ranges = _variable_ranges(fd, name)
        buf = np.empty(sum(n for _, n in ranges), dtype=np.uint8)
        pos = 0
        for off, n in ranges:
            if n:
                _pread_into(fd, buf[pos:pos + n], off)
            pos += n
    finally:
        os.close(fd)
    return buf.view(_file_dtype(v)).reshape(v['shape']), v['dims'], dict(v['attrs'])


def update_variable(path, name, values):
    """Overwrite the data of the existing variable `name` of a NetCDF-3 file with `values`: `os.pwrite` at the offsets the
    header gives (fixed-size and record variables), in the file's byte order - big-endian values go out as they are, native
    ones are swapped in one pass.  `values` must have the variable's shape and its type (kind and size; either byte order).
    Every other byte of the file stays as it was; the file is neither rewritten nor resized.  KeyError for an unknown
    variable, ValueError for a shape or dtype that differs; nothing is written then."""
    import os
    values = np.asarray(values)
    fd = os.open(path, os.O_RDWR)
    try:
        v, ranges = _variable_ranges(fd, name)
        if (values.dtype.kind, values.dtype.itemsize) != (v['dtype'].kind, v['dtype'].itemsize):
            raise ValueError('variable %s is stored as %s, got values of dtype %s' % (name, v['dtype'], values.dtype))
        if tuple(values.shape) != tuple(v['shape']):
            raise ValueError('variable %s has shape %s, got values of shape %s' % (name, tuple(v['shape']), tuple(values.shape)))
        flat = np.ascontiguousarray(values).astype(_file_dtype(v), copy=False).reshape(-1).view(np.uint8)
        pos = 0
        for off, n in ranges:
            mv = memoryview(flat[pos:pos + n])
            pos += n
            while len(mv):
                done = os.pwrite(fd, mv, off)
                off += done
                mv = mv[done:]
    finally:
        os.close(fd)


# ------------------------------------------------------------------------------ band-wise I/O (latency mode)
# One ERA5 file over several ranks in latitude bands: every rank reads and writes only its
# rows of the fields.  In the classic layout a variable (..., lat, lon) is C-ordered, so rows [j0, j1) of one (time, level)
# plane are ONE contiguous byte range: a band is one pread / pwrite per plane.
def _band_ranges(v, recsize, numrecs, j0, j1, lat_axis):
    """(outer index tuple, file offset, byte count) of the rows [j0, j1) of every plane of a variable described by a
    header entry `v` (shape, dtype, begin, record); lat_axis counts from the end (-2: (..., lat, lon))."""
    shape = list(v['shape'])
    nd = len(shape)
    ax = nd + lat_axis
    if ax < 0 or nd < 2:
        raise ValueError('variable %s has no latitude axis' % v['name'])
    item = v['dtype'].itemsize
    inner = int(np.prod(shape[ax + 1:], dtype=np.int64))          # elements per latitude row
    nlat = shape[ax]
    outer = shape[:ax]
    out = []
    for idx in np.ndindex(*outer) if outer else [()]:
        if v['record']:
            r, rest = idx[0], idx[1:]
            lin = 0
            for n, i in zip(shape[1:ax], rest):
                lin = lin * n + i
            off = v['begin'] + r * recsize + (lin * nlat + j0) * inner * item
        else:
            lin = 0
            for n, i in zip(outer, idx):
                lin = lin * n + i
            off = v['begin'] + (lin * nlat + j0) * inner * item
        out.append((idx, off, (j1 - j0) * inner * item))
    return out


def read_band(path, name, j0, j1, lat_axis=-2, hdr=None):
    """Rows [j0, j1) along the latitude axis of variable `name`: array of the variable's shape with that axis cut to
    j1 - j0, native byte order; one `pread` per (time, level) plane."""
    import os
    fd = os.open(path, os.O_RDONLY)
    try:
        if hdr is None:
            hdr = _parse_header(fd, os.fstat(fd).st_size)
        v = {x['name']: x for x in hdr['vars']}[name]
        shape = list(v['shape'])
        ax = len(shape) + lat_axis
        shape[ax] = j1 - j0
        out = np.empty(shape, dtype=v['dtype'].newbyteorder('>') if v['dtype'].itemsize > 1 else v['dtype'])
        for idx, off, nbytes in _band_ranges(v, hdr['recsize'], hdr['numrecs'], j0, j1, lat_axis):
            if nbytes:
                _pread_into(fd, out[idx].reshape(-1).view(np.uint8), off)
    finally:
        os.close(fd)
    return out.astype(v['dtype']) if v['dtype'].itemsize > 1 else out


class BandedWriter:
    """An output file several ranks write together: `template` is the Dataset to be written, `banded` the names of the
    variables every rank holds only a latitude band of (placeholders in the template).  Rank 0 calls `create()` - header,
    file size, every other variable; after a barrier each rank calls `write_band(name, j0, j1, rows)` for its rows of
    every banded variable.  The result is byte for byte the file to_netcdf writes from the whole arrays."""

    def __init__(self, template, path, banded, lat_axis=-2):
        self.ds, self.path, self.banded, self.lat_axis = template, path, tuple(banded), lat_axis
        hdr, specs, begins, total, recsize, numrecs = _plan(template)
        self._recsize, self._numrecs = recsize, numrecs
        self._vars = {}
        for sp, b in zip(specs, begins):
            if sp['name'] in self.banded:
                self._vars[sp['name']] = dict(name=sp['name'], shape=list(sp['data'].shape), dtype=np.dtype(sp['data'].dtype.str[1:]),
                                              begin=b, record=sp['record'])

    def create(self, threads=None):
        to_netcdf(self.ds, self.path, threads=threads, skip=self.banded)

    def write_band(self, name, j0, j1, rows):
        import os
        v = self._vars[name]
        rows = np.asarray(rows)
        want = list(v['shape'])
        want[len(want) + self.lat_axis] = j1 - j0
        if list(rows.shape) != want:
            raise ValueError('band of %s has shape %s, expected %s' % (name, rows.shape, want))
        big = np.ascontiguousarray(rows.astype(v['dtype'].newbyteorder('>'), copy=False))
        fd = os.open(self.path, os.O_WRONLY)
        try:
            for idx, off, nbytes in _band_ranges(v, self._recsize, self._numrecs, j0, j1, self.lat_axis):
                mv = memoryview(np.ascontiguousarray(big[idx]).reshape(-1).view(np.uint8))
                while len(mv):
                    n = os.pwrite(fd, mv, off)
                    off += n
                    mv = mv[n:]
        finally:
            os.close(fd)


def _to_netcdf_scipy(ds, path):
    """Write a Dataset as NetCDF-3 64-bit-offset (`.to_netcdf(path, mode='w')`, step_03:378)."""
    nc = netcdf_file(path, 'w', version=2)
    for k, v in ds.attrs.items():
        setattr(nc, k, v)
    made = {}
    for f in ds.variables.values():
        for d, n in zip(f.dims, f.shape):
            if d not in made:
                nc.createDimension(d, int(n))
                made[d] = n
    for name, f in ds.variables.items():
        data = f.values
        attrs = dict(f.attrs)
        if data.dtype.kind == 'M':
            data = (data.astype('datetime64[s]') - np.datetime64('1970-01-01T00:00:00', 's')).astype(np.float64)
            attrs['units'] = 'seconds since 1970-01-01 00:00:00'
            attrs['calendar'] = 'proleptic_gregorian'
        if data.dtype == np.int64:
            data = data.astype(np.int32)
        if data.dtype == np.bool_:
            data = data.astype(np.int8)
        var = nc.createVariable(name, data.dtype.newbyteorder('='), f.dims)
        var[...] = data
        for k, v in attrs.items():
            if k in ('_FillValue',) and np.ndim(v) == 0:
                v = np.asarray(v, dtype=data.dtype)
            setattr(var, k, v)
    nc.close()
