"""CPU tests of postproc_cosmo.extpar_adapt: the per-cell rule of `pgw_time_mean_add` against the numpy expression it
restates (tests/extpar_cases.py), the condition under which bit-for-bit comparisons can tell the dtype flows apart, the
in-place update of one NetCDF variable (`ncio.update_variable`), the command line, and the errors that are raised before a
device context exists and before a byte of the file changes."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import extpar_cases as E                                                             # noqa: E402
from pgw4era5_amd import ncio, synthetic                                             # noqa: E402


# ---- the rule and the numpy expression -----------------------------------------------------------------------------------
@pytest.mark.parametrize('pair', E.PAIRS, ids=lambda p: '%s+=%s' % p)
@pytest.mark.parametrize('mask', E.MASKS)
def test_per_cell_rule_is_the_numpy_expression(pair, mask):
    tb, tx = pair
    for pattern in E.NAN_PATTERNS:
        for nrec in (1, 12):
            x = E.records(nrec, 65, tx, pattern)
            base, mv = E.base_and_mask(65, tb, mask)
            out, mean, n_masked, n_new_nan = E.statement(base, x, mv)
            lo, lm = E.python_loop(base, x, mv)
            what = (pattern, nrec)
            assert E.same_bits(lm, mean), what
            assert E.same_bits(lo, out, raw=E.mask_of(base, mv)), what
            assert out.dtype == tb and mean.dtype == tx
            if mask == 'every_cell':
                assert n_masked == 65 and n_new_nan == 0
            if pattern == 'all_records_of_a_cell' and mask == 'none':
                assert n_new_nan == int(np.isnan(mean).sum()) > 0
            if pattern == 'negative_zeros':
                if nrec > 1:
                    cell = np.nonzero((x == 0).any(axis=0) & np.isnan(x).any(axis=0))[0][0]
                    assert not np.signbit(mean[cell]) and mean[cell] == 0     # a NaN record adds +0.0
                assert not np.signbit(mean[0]) and mean[0] == 0               # ... and so does the identity the sum starts from


@pytest.mark.parametrize('tx', [E.F32, E.F64], ids=str)
def test_one_cell_is_numpys_pairwise_sum(tx):
    """A grid of one cell: the records lie contiguous and numpy adds them pairwise - another result than record order from
    8 records on.  Around the block sizes of numpy's pairwise_sum (8, 128) and past its first split."""
    differs = 0
    for nrec in E.N_REC + [7, 16, 17, 127, 128, 129, 136, 300, 1000]:
        for pattern in ('none', 'one_record_of_a_cell', 'negative_zeros'):
            x = E.records(nrec, 1, tx, pattern)
            base, mv = E.base_and_mask(1, E.F32, 'none')
            out, mean, _, _ = E.statement(base, x, mv)
            lo, lm = E.python_loop(base, x, mv)
            assert E.same_bits(lm, mean) and E.same_bits(lo, out), (nrec, pattern)
            in_order = tx.type(0.0)
            for v in np.where(np.isnan(x[:, 0]), tx.type(0.0), x[:, 0]):
                in_order = tx.type(in_order + v)
            differs += int(in_order / tx.type(max(nrec, 1)) != mean[0]) if pattern == 'none' else 0
    assert differs >= 5                                                      # the two orders are told apart


def test_leading_axes_of_length_one_and_the_squeeze():
    x = E.records(12, 63, E.F32).reshape(12, 7, 9)
    base, mv = E.base_and_mask(63, E.F32, 'one_value')
    flat = E.statement(base, x.reshape(12, 63), mv)[0]
    assert E.same_bits(E.statement(base.reshape(1, 7, 9), x, mv)[0].reshape(-1), flat)
    assert E.same_bits(E.statement(base.reshape(7, 9), x, mv)[0].reshape(-1), flat)


def test_the_data_can_tell_the_flows_apart():
    """float32 record-order sum against the float64 sum rounded once, record order against reversed order, the latter for
    float64 data too: each differs in at least a quarter of the cells, or the GPU comparisons would prove little."""
    shares = E.check_data_tells_flows_apart()
    print('shares of differing cells: f32 sum vs f64 sum %.3f, f32 order %.3f, f64 order %.3f' % shares)
    assert len(shares) == 3 and min(shares) >= 0.25
    # ... and through the whole statement: the float64-accumulating mean is another result in many cells
    x = E.records(12, 1032, E.F32)
    other = (x.astype(E.F64).sum(axis=0) / 12).astype(E.F32)
    assert (E.uview(E.nanmean(x)) != E.uview(other)).mean() >= 0.125


# ---- ncio.update_variable ------------------------------------------------------------------------------------------------
def _file(tmp_path, dtype, record):
    F = ncio.Field
    rng = np.random.default_rng(3)
    ds = ncio.Dataset(attrs=dict(title='update_variable'), record_dim='time' if record else None)
    ds['time'] = F(np.arange(3, dtype=np.float64), ('time',))
    ds['y'] = F(np.arange(5, dtype=np.float64), ('y',))
    ds['before'] = F(rng.standard_normal((3, 5, 7)).astype(np.float32), ('time', 'y', 'x'))
    ds['var'] = F(rng.standard_normal((3, 5, 7)).astype(dtype), ('time', 'y', 'x'), attrs=dict(units='K'))
    ds['odd'] = F(rng.integers(0, 100, (3, 5)).astype(np.int16), ('time', 'y'))          # 10 bytes per record: padded
    ds['fixed'] = F(rng.standard_normal((5, 7)).astype(dtype), ('y', 'x'))
    ds['after'] = F(rng.standard_normal((5, 7)), ('y', 'x'))
    path = str(tmp_path / 'f.nc')
    ncio.to_netcdf(ds, path)
    return path, ds


@pytest.mark.parametrize('dtype', ['float32', 'float64'])
@pytest.mark.parametrize('record', [False, True], ids=['fixed', 'record'])
def test_update_variable_writes_the_variable_and_nothing_else(tmp_path, dtype, record):
    path, ds = _file(tmp_path, dtype, record)
    before = open(path, 'rb').read()
    rng = np.random.default_rng(9)
    for name, order in (('var', '='), ('fixed', '>')):                   # native values, and values in the file's byte order
        raw, dims, attrs = ncio.read_variable_raw(path, name)
        assert raw.dtype == np.dtype(dtype).newbyteorder('>') and dims == ds[name].dims
        assert np.array_equal(raw.astype(dtype), ds[name].values)
        new = rng.standard_normal(ds[name].shape).astype(np.dtype(dtype).newbyteorder(order))
        old_bytes = raw.tobytes()
        ncio.update_variable(path, name, new)
        after = open(path, 'rb').read()
        assert len(after) == len(before)
        got = ncio.open_dataset(path)
        assert np.array_equal(got[name].values, new.astype(dtype)) and got[name].values.dtype == np.dtype(dtype)
        # every byte that differs lies in the variable's data: putting the old words back restores the file
        ncio.update_variable(path, name, np.frombuffer(old_bytes, dtype=raw.dtype).reshape(raw.shape))
        assert open(path, 'rb').read() == before
        ncio.update_variable(path, name, new)
        changed = np.nonzero(np.frombuffer(open(path, 'rb').read(), np.uint8) != np.frombuffer(before, np.uint8))[0]
        assert 0 < len(changed) <= new.nbytes
        for other in ds.variables:
            if other != name:
                assert np.array_equal(got[other].values, ncio.open_dataset(path)[other].values), other
        before = open(path, 'rb').read()
    if record:
        assert ncio.open_dataset(path).record_dim == 'time'


def test_update_variable_refuses_what_does_not_fit(tmp_path):
    path, ds = _file(tmp_path, 'float32', True)
    before = open(path, 'rb').read()
    with pytest.raises(ValueError, match='shape'):
        ncio.update_variable(path, 'var', np.zeros((3, 5, 6), np.float32))
    with pytest.raises(ValueError, match='shape'):
        ncio.update_variable(path, 'var', np.zeros((5, 7), np.float32))
    with pytest.raises(ValueError, match='dtype'):
        ncio.update_variable(path, 'var', np.zeros((3, 5, 7), np.float64))
    with pytest.raises(ValueError, match='dtype'):
        ncio.update_variable(path, 'var', np.zeros((3, 5, 7), np.int32))
    with pytest.raises(KeyError):
        ncio.update_variable(path, 'nothing', np.zeros((3, 5, 7), np.float32))
    with pytest.raises(KeyError):
        ncio.read_variable_raw(path, 'nothing')
    assert open(path, 'rb').read() == before


# ---- synthetic.make_extpar -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('fill', ['_FillValue', 'missing_value', 'both', None])
def test_make_extpar(tmp_path, fill):
    from pgw4era5_amd.postproc_cosmo import extpar_adapt as A
    info = synthetic.make_extpar(str(tmp_path / 'extpar.nc'), dtype=np.float64, time_axis=True, fill=fill)
    ds = ncio.open_dataset(info['path'], decode_times=False)
    assert ds['T_CL'].dims == ('time', 'rlat', 'rlon') and ds['T_CL'].shape == (1, 7, 9) and ds['T_CL'].dtype == np.float64
    assert ds['lat'].dims == ('rlat', 'rlon') and ds['lon'].shape == (7, 9)
    raw, dims, attrs = ncio.read_variable_raw(info['path'], 'T_CL')
    assert A.mask_values(attrs) == info['mask_values'] and len(info['mask_values']) == (2 if fill == 'both' else 1)
    assert np.array_equal(E.mask_of(raw.astype('f8'), A.mask_values(attrs)), info['masked']) and 0 < info['masked'].sum() < 63
    assert ('_FillValue' in attrs) == (fill in ('_FillValue', 'both'))
    assert ('missing_value' in attrs) == (fill in ('missing_value', 'both'))


# ---- command line --------------------------------------------------------------------------------------------------------
def test_command_line_surface(capsys):
    from pgw4era5_amd.postproc_cosmo import extpar_adapt as A
    assert A.var_name_map == {'ts': 'T_CL'}
    args = A.parse_args(['ext.nc', '-d', 'deltas'])
    assert args.extpar_file_path == 'ext.nc' and args.delta_input_dir == 'deltas'
    assert A.parse_args(['--delta_input_dir', 'd2', 'e2.nc']).delta_input_dir == 'd2'
    assert A.parse_args(['ext.nc']).delta_input_dir is None
    with pytest.raises(SystemExit) as e:
        A.parse_args(['--help'])
    assert e.value.code == 0
    text = capsys.readouterr().out
    assert 'T_CL' in text and 'delta_input_dir' in text and 'extpar_file_path' in text
    for bad in (['ext.nc', '--bands'], ['ext.nc', '-o', 'x'], [], ['a.nc', 'b.nc']):
        with pytest.raises(SystemExit) as e:
            A.parse_args(bad)
        assert e.value.code != 0


# ---- errors before the device and before the file changes ----------------------------------------------------------------
class _NoDevice:
    """default_context replaced: a call that reaches the device layer fails the test."""

    def __call__(self):
        raise AssertionError('the device was reached')


def _delta_dir(tmp_path, shape=(7, 9), name='ts'):
    d = tmp_path / ('deltas_%dx%d_%s' % (shape + (name,)))
    d.mkdir()
    F = ncio.Field
    ds = ncio.Dataset()
    days = (np.array(['1995-%02d-15' % (m + 1) for m in range(12)], dtype='datetime64[D]') - np.datetime64('1850-01-01')).astype(np.float64)
    ds['time'] = F(days, ('time',), attrs=dict(units='days since 1850-01-01 00:00:00', calendar='proleptic_gregorian'))
    ds[name] = F(E.records(12, shape[0] * shape[1], E.F32).reshape((12,) + shape), ('time', 'rlat', 'rlon'))
    ncio.to_netcdf(ds, str(d / 'ts_delta.nc'))
    return str(d)


@pytest.fixture
def no_device(monkeypatch):
    from pgw4era5_amd import device, functions
    from pgw4era5_amd.postproc_cosmo import extpar_adapt as A
    for mod in (device, functions, A):
        monkeypatch.setattr(mod, 'default_context', _NoDevice())
    return A


def test_errors_leave_the_file_alone_and_the_device_untouched(tmp_path, no_device):
    A = no_device
    info = synthetic.make_extpar(str(tmp_path / 'extpar.nc'))
    path = info['path']
    before = open(path, 'rb').read()
    good = _delta_dir(tmp_path)
    with pytest.raises(ValueError, match=r'\(-d\) is required'):
        A.extpar_adapt(path, None)
    with pytest.raises(ValueError, match=r'\(-d\) is required'):
        A.main([path])
    with pytest.raises(ValueError, match='not on the same grid'):
        A.extpar_adapt(path, _delta_dir(tmp_path, (7, 8)))
    with pytest.raises(ValueError, match='not on the same grid'):
        A.extpar_adapt(path, _delta_dir(tmp_path, (9, 7)))
    assert open(path, 'rb').read() == before
    # a file without T_CL
    ds = ncio.open_dataset(path, decode_times=False, decode_mask_scale=False)
    t_cl = ds['T_CL']
    del ds['T_CL']
    other = str(tmp_path / 'no_t_cl.nc')
    ncio.to_netcdf(ds, other)
    kept = open(other, 'rb').read()
    with pytest.raises(ValueError, match='no variable T_CL'):
        A.extpar_adapt(other, good)
    assert open(other, 'rb').read() == kept
    # a packed T_CL
    packed = str(tmp_path / 'packed.nc')
    ds['T_CL'] = ncio.Field(np.round((t_cl.values - 280.0) / 0.01).clip(-32000, 32000).astype(np.int16), t_cl.dims,
                            attrs=dict(scale_factor=np.float32(0.01), add_offset=np.float32(280.0)))
    ncio.to_netcdf(ds, packed)
    kept = open(packed, 'rb').read()
    with pytest.raises(ValueError, match='packed'):
        A.extpar_adapt(packed, good)
    assert open(packed, 'rb').read() == kept


def test_function_level_shape_errors_come_before_the_device(no_device):
    from pgw4era5_amd import functions as F
    x = E.records(12, 63, E.F32).reshape(12, 7, 9)
    base = np.zeros((7, 9), np.float32)
    for bad in (np.zeros((9, 7), np.float32), np.zeros((2, 7, 9), np.float32), np.zeros((7, 9, 1), np.float32), np.zeros(9, np.float32),
                np.zeros((7, 1, 9), np.float32)):
        with pytest.raises(ValueError, match='does not take the mean'):
            F.time_mean_add(bad, x)
    with pytest.raises(ValueError, match='at most two'):
        F.time_mean_add(base, x, mask_values=[1.0, 2.0, 3.0])
    with pytest.raises(ValueError, match='at least one record'):
        F.time_mean(np.zeros((0, 7, 9), np.float32))
    with pytest.raises(ValueError):
        F.time_mean(np.float32(1.0))
    with pytest.raises(ValueError, match='no cells'):
        F.time_mean(np.zeros((3, 0), np.float32))
    with pytest.raises(ValueError, match='out must be'):
        F.time_mean_add(base, x, out=base)
