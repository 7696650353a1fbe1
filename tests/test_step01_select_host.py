"""CPU checks of the host side of step_01's level selection, lon-lat box and model-top merge
(pgw4era5_amd/step_01_extract_deltas.py: lonlat_box, level_indices, the sub-commands `select`, `merge_levels` and
`climatology -b`) and of the declaration of `pgw_select_box`.  `cdo` is not available, so the definitions in the
docstrings of `lonlat_box` and `level_indices` are the contract; the expected indices below are worked out by hand."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def s1():
    from pgw4era5_amd import step_01_extract_deltas
    return step_01_extract_deltas


LON360 = np.arange(0.0, 360.0, 10.0)                  # 36 columns, 0 ... 350
LON180 = np.arange(-180.0, 180.0, 10.0)               # 36 columns, -180 ... 170
LAT_NS = np.arange(85.0, -90.0, -10.0)                # 18 rows, 85 ... -85 (north to south)
LAT_SN = LAT_NS[::-1].copy()


def cols_of(lon0, n, nlon):
    return (lon0 + np.arange(n)) % nlon


def test_select_box_is_declared_and_bound_without_a_profile_id():
    from pgw4era5_amd import _lib
    hdr = open(os.path.join(ROOT, 'include', 'pgw_hip.h')).read()
    assert 'pgw_select_box' in _lib.SIGNATURES and 'int pgw_select_box(' in hdr
    res, args = _lib.SIGNATURES['pgw_select_box']
    assert len(args) == 16
    assert len(_lib.KERNEL_IDS) == 28 and 'PGW_K_COUNT = 28' in hdr
    # the entry cites the script lines it replaces
    for cite in ('extract_climate_delta.sh:194-208', 'CFday_cut_subdomain.sh:28-30', 'Emon_add_top_from_Amon.sh:45-56'):
        assert cite in hdr


def test_box_wraps_across_zero_on_a_0_360_grid(s1):
    # -73 ... 37: columns 290 (-70), ..., 350 (-10), then 0 ... 30
    lat0, nlat, lon0, nlon, lon_out = s1.lonlat_box(LAT_NS, LON360, (-73, 37, -42, 34))
    assert (lon0, nlon) == (29, 11)
    assert np.array_equal(lon_out, np.arange(-70.0, 31.0, 10.0))
    assert np.all(np.diff(lon_out) > 0) and lon_out[0] < 0 < lon_out[-1]
    assert np.array_equal(LON360[cols_of(lon0, nlon, 36)] % 360, lon_out % 360)
    # rows 25, 15, 5, -5, ..., -35: indices 6 ... 12 of the north-to-south axis
    assert (lat0, nlat) == (6, 7)
    assert np.array_equal(LAT_NS[lat0:lat0 + nlat], np.arange(25.0, -36.0, -10.0))


def test_box_without_wrap(s1):
    lat0, nlat, lon0, nlon, lon_out = s1.lonlat_box(LAT_NS, LON360, (95, 205, 0, 90))
    assert (lon0, nlon) == (10, 11) and np.array_equal(lon_out, np.arange(100.0, 201.0, 10.0))
    assert (lat0, nlat) == (0, 9)


def test_identity_and_rotations(s1):
    lat0, nlat, lon0, nlon, lon_out = s1.lonlat_box(LAT_NS, LON360, (0, 360, -90, 90))
    assert (lat0, nlat, lon0, nlon) == (0, 18, 0, 36) and np.array_equal(lon_out, LON360)
    # -180 ... 180 on 0 ... <360: starts at column 180, which is shifted to -180; 360-degree span: every column once
    _, _, lon0, nlon, lon_out = s1.lonlat_box(LAT_NS, LON360, (-180, 180, -90, 90))
    assert (lon0, nlon) == (18, 36) and np.array_equal(lon_out, LON180)
    # 0 ... 360 on -180 ... <180: starts at column 0 deg; the western half moves behind the eastern one
    _, _, lon0, nlon, lon_out = s1.lonlat_box(LAT_NS, LON180, (0, 360, -90, 90))
    assert (lon0, nlon) == (18, 36) and np.array_equal(lon_out, LON360)


def test_columns_and_rows_on_the_bounds_are_included(s1):
    lat0, nlat, lon0, nlon, lon_out = s1.lonlat_box(LAT_NS, LON360, (-70, 30, -35, 25))
    assert (lon0, nlon) == (29, 11) and lon_out[0] == -70.0 and lon_out[-1] == 30.0
    assert (lat0, nlat) == (6, 7)
    # just inside the same columns / rows: they drop out
    _, nlat2, lon02, nlon2, _ = s1.lonlat_box(LAT_NS, LON360, (-69.999, 29.999, -34.999, 24.999))
    assert (lon02, nlon2) == (30, 9) and nlat2 == 5
    # a 360-degree span whose bounds both fall on one column: the smallest k wins, the column appears once, first
    _, _, lon0, nlon, lon_out = s1.lonlat_box(LAT_NS, LON360, (-10, 350, -90, 90))
    assert (lon0, nlon) == (35, 36) and lon_out[0] == -10.0 and lon_out[-1] == 340.0
    # a single column
    _, _, lon0, nlon, lon_out = s1.lonlat_box(LAT_NS, LON360, (-1, 1, -90, 90))
    assert (lon0, nlon) == (0, 1) and lon_out[0] == 0.0


def test_both_latitude_orders_and_swapped_latitude_bounds(s1):
    a = s1.lonlat_box(LAT_NS, LON360, (0, 100, -42, 34))
    b = s1.lonlat_box(LAT_NS, LON360, (0, 100, 34, -42))
    assert a[:4] == b[:4] == (6, 7, 0, 11)
    lat0, nlat = s1.lonlat_box(LAT_SN, LON360, (0, 100, -42, 34))[:2]
    assert (lat0, nlat) == (5, 7)
    assert np.array_equal(LAT_SN[lat0:lat0 + nlat], np.arange(-35.0, 26.0, 10.0))


def test_lon_out_keeps_a_float32_coordinate_dtype(s1):
    out = s1.lonlat_box(LAT_NS.astype(np.float32), LON360.astype(np.float32), (-73, 37, -42, 34))[4]
    assert out.dtype == np.float32 and out[0] == np.float32(-70.0)
    assert s1.lonlat_box(LAT_NS, LON360.astype(np.int32), (-73, 37, -42, 34))[4].dtype == np.float64


def test_box_errors(s1):
    lat2d, lon2d = np.meshgrid(LAT_NS, LON360, indexing='ij')
    with pytest.raises(ValueError, match='2-D'):
        s1.lonlat_box(lat2d, lon2d, (0, 10, 0, 10))
    with pytest.raises(ValueError, match='ascending'):
        s1.lonlat_box(LAT_NS, LON360[::-1], (0, 100, 0, 10))
    with pytest.raises(ValueError, match='ascending'):
        s1.lonlat_box(LAT_NS, np.array([0.0, 10.0, 10.0, 20.0]), (0, 100, 0, 10))
    with pytest.raises(ValueError, match='lon1 < lon2'):
        s1.lonlat_box(LAT_NS, LON360, (37, -73, -42, 34))
    with pytest.raises(ValueError, match='lon1 < lon2'):
        s1.lonlat_box(LAT_NS, LON360, (10, 10, -42, 34))
    with pytest.raises(ValueError, match='360'):
        s1.lonlat_box(LAT_NS, LON360, (0, 361, -42, 34))
    with pytest.raises(ValueError, match='box must be'):
        s1.lonlat_box(LAT_NS, LON360, (0, 100, 0))
    with pytest.raises(ValueError, match='monotonic'):
        s1.lonlat_box(np.array([10.0, 50.0, 20.0, 60.0]), LON360, (0, 100, 0, 30))
    with pytest.raises(ValueError, match='no latitude'):
        s1.lonlat_box(LAT_NS, LON360, (0, 100, 1, 4))
    with pytest.raises(ValueError, match='no longitude'):
        s1.lonlat_box(LAT_NS, LON360, (1, 9, -42, 34))


def test_level_indices_keep_the_file_order(s1):
    plev = np.array([100000.0, 85000.0, 50000.0, 25000.0, 10000.0, 5000.0])
    idx = s1.level_indices(plev, [5000, 100000, 50000])              # a shuffled request
    assert idx.tolist() == [0, 2, 5] and idx.dtype == np.int32
    assert s1.level_indices(plev[::-1], [5000, 100000, 50000]).tolist() == [0, 3, 5]
    assert s1.level_indices(plev.astype(np.float32), plev.tolist()).tolist() == list(range(6))
    assert s1.level_indices(plev, 25000).tolist() == [3]
    with pytest.raises(ValueError, match='70000'):
        s1.level_indices(plev, [100000, 70000])
    with pytest.raises(ValueError, match='twice'):
        s1.level_indices(plev, [100000, 5000, 100000])
    with pytest.raises(ValueError):
        s1.level_indices(plev, [])


def test_argument_surface_of_the_new_sub_commands(s1):
    p = s1.build_parser()
    a = p.parse_args(s1._join_box_option(['select', '-i', 'in_{}.nc', '-o', 'out_{}.nc', '-v', 'ta,hur', '-l', '100000,85000',
                                          '-b', '-73,37,-42,34', '--max_records', '3']))
    assert (a.command, a.input, a.output, a.var_names, a.max_records) == ('select', 'in_{}.nc', 'out_{}.nc', 'ta,hur', 3)
    assert s1._parse_floats(a.levels, 'levels') == [100000.0, 85000.0]
    assert s1._parse_floats(a.box, 'box', 4) == [-73.0, 37.0, -42.0, 34.0]
    a = p.parse_args(['select', '-i', 'a', '-o', 'b', '-v', 'ta', '--box=0,360,-90,90'])
    assert a.box == '0,360,-90,90' and a.levels is None and a.max_records is None
    m = p.parse_args(['merge_levels', 'emon_{}.nc', 'amon_{}.nc', 'out_{}.nc', '-v', 'ua,va', '--levels_a', '100000,97500',
                      '--levels_b', '7000,5000'])
    assert (m.command, m.file_a, m.file_b, m.out_file, m.var_names) == ('merge_levels', 'emon_{}.nc', 'amon_{}.nc', 'out_{}.nc', 'ua,va')
    assert s1._parse_floats(m.levels_b, 'levels_b') == [7000.0, 5000.0]
    m = p.parse_args(['merge_levels', 'a', 'b', 'c', '-v', 'ta'])
    assert m.levels_a is None and m.levels_b is None
    c = p.parse_args(s1._join_box_option(['climatology', '-i', 'a.nc', '-o', 'b.nc', '-v', 'ta', '-m', 'ymonmean', '-b', '-73,37,-42,34']))
    assert c.command == 'climatology' and c.box == '-73,37,-42,34'
    assert p.parse_args(['climatology', '-i', 'a.nc', '-o', 'b.nc', '-v', 'ta', '-m', 'ymonmean']).box is None
    with pytest.raises(ValueError, match='4'):
        s1._parse_floats('1,2,3', 'box', 4)
    with pytest.raises(ValueError, match='numbers'):
        s1._parse_floats('1,x', 'levels')
    with pytest.raises(SystemExit):
        p.parse_args(['select', '-o', 'b', '-v', 'ta'])
    with pytest.raises(SystemExit):
        p.parse_args(['merge_levels', 'a', 'b', '-v', 'ta'])
    # the earlier sub-commands parse as before, and `delta` is dispatched by name
    d = p.parse_args(['delta', 's.nc', 'h.nc', 'd.nc', '-v', 'ta'])
    assert d.command == 'delta'
    with pytest.raises(ValueError, match='needs --levels'):
        s1.main(['select', '-i', 'a.nc', '-o', 'b.nc', '-v', 'ta'])


def test_help_of_the_new_sub_commands_runs_without_the_library():
    env = dict(os.environ, PGW_LIB=os.path.join(ROOT, 'no_such_dir', 'libpgw_hip.so'), PYTHONPATH=ROOT)
    for argv in (['select', '--help'], ['merge_levels', '--help'], ['climatology', '--help']):
        r = subprocess.run([sys.executable, '-m', 'pgw4era5_amd.step_01_extract_deltas'] + argv, cwd=ROOT, env=env,
                           capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        assert 'usage' in r.stdout
        if argv[0] != 'merge_levels':
            assert '--box' in r.stdout
