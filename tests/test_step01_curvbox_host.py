"""CPU checks of step_01's lon-lat box on curvilinear grids: the numpy statement itself (tests/curvbox_cases.py) by hand,
the window rule and the `auto` detection of pgw4era5_amd/step_01_extract_deltas.py against it, the conditions the shared
cases must fulfil so that no GPU test passes on an empty or trivial selection, and the errors raised before the device is
touched."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import curvbox_cases as C                                                             # noqa: E402


@pytest.fixture(scope='module')
def s1():
    from pgw4era5_amd import step_01_extract_deltas
    return step_01_extract_deltas


@pytest.fixture()
def no_device(s1, monkeypatch):
    """Any use of the device fails the test."""
    def boom(*a, **k):
        raise AssertionError('the device was touched')
    monkeypatch.setattr(s1, 'default_context', boom)


# ------------------------------------------------------------------------------- 1. the statement by hand
def test_statement_by_hand():
    lat = np.array([[50.0, 34.0, 34.5, -10.0],
                    [0.0, -42.0, np.nan, 10.0],
                    [-60.0, -43.0, 20.0, np.inf]])
    lon = np.array([[0.0, 37.0, 10.0, 38.0],
                    [287.0, 300.0, 5.0, -433.0],
                    [0.0, 0.0, 650.0, 0.0]])
    # box -73 ... 37, -42 ... 34:
    # row 0: lat 50 out | on lat2 and lon2: in | lat 34.5 out | lon 38 -> k = 0, 38 > 37: out
    # row 1: 287 - 360 = -73 on lon1: in | 300 - 360 = -60, lat on lat1: in | NaN lat: out | -433 + 360 = -73: in
    # row 2: lat -60 out | lat -43 out | 650 - 720 = -70: in | inf lat: out
    want = np.array([[0, 1, 0, 0], [1, 1, 0, 1], [0, 0, 1, 0]], dtype=bool)
    assert np.array_equal(C.inside_ref(lat, lon, C.REF_BOX), want)
    assert np.array_equal(C.inside_ref(lat, lon, (-73.0, 37.0, 34.0, -42.0)), want)          # lat1 > lat2: the same band
    row_any, col_any, n = C.flags_ref(lat, lon, C.REF_BOX)
    assert row_any.tolist() == [1, 1, 1] and col_any.tolist() == [1, 1, 1, 1] and n == 5
    assert np.array_equal(C.inside_ref(lat.astype(np.float32), lon.astype(np.float32), C.REF_BOX), want)
    # the rectangle: all three rows; all columns flagged -> (0, 4) either way
    assert C.box_ref(lat, lon, C.REF_BOX, cyclic=True) == (0, 3, 0, 4, 5)
    assert C.box_ref(lat, lon, C.REF_BOX, cyclic=False) == (0, 3, 0, 4, 5)
    # the whole circle: every cell with finite coordinates in the band
    assert C.flags_ref(lat, lon, C.GLOBAL_BOX)[2] == 10


# ------------------------------------------------------------------------------- 2. the window rule
def cols(ni, on):
    c = np.zeros(ni, dtype=np.int32)
    c[list(on)] = 1
    return c


WINDOW_CASES = [
    # (row flags, column flags, cyclic window, plain window)
    ([0, 1, 0, 1, 0], cols(8, [2, 6]), (1, 3, 6, 5), (1, 3, 2, 5)),          # tie of two runs of 3 (3..5, 7..1): lowest start 3
    ([1], cols(8, [0, 4]), (0, 1, 4, 5), (0, 1, 0, 5)),                      # tie 1..3 and 5..7: the run from 1 is dropped
    ([1, 1], cols(6, range(6)), (0, 2, 0, 6), (0, 2, 0, 6)),                 # all columns flagged
    ([0, 0, 1], cols(7, [0]), (2, 1, 0, 1), (2, 1, 0, 1)),                   # a single column at index 0
    ([1, 0, 0], cols(7, [6]), (0, 1, 6, 1), (0, 1, 6, 1)),                   # ... and at index ni - 1
    ([1, 1, 1], cols(10, [0, 1, 8, 9]), (0, 3, 8, 4), (0, 3, 0, 10)),        # across the seam
    ([1, 1, 1], cols(10, [0, 1, 4, 9]), (0, 3, 9, 6), (0, 3, 0, 10)),        # unflagged runs 2..3 and 5..8: the longer goes
    ([1], cols(1, [0]), (0, 1, 0, 1), (0, 1, 0, 1)),
]


@pytest.mark.parametrize('case', range(len(WINDOW_CASES)))
def test_window_rule(s1, case):
    rows, c, want_cyclic, want_plain = WINDOW_CASES[case]
    assert C.windows_ref(rows, c, True) == want_cyclic and C.windows_ref(rows, c, False) == want_plain
    assert s1.flag_windows(np.array(rows, dtype=np.int32), c, True) == want_cyclic
    assert s1.flag_windows(np.array(rows, dtype=np.int32), c, False) == want_plain


def test_window_rule_random(s1):
    rng = np.random.default_rng(3)
    n = 0
    for ni in (1, 2, 3, 5, 8, 13, 64):
        for _ in range(40):
            c = (rng.random(ni) < rng.choice([0.15, 0.5, 0.9])).astype(np.int32)
            r = (rng.random(6) < 0.5).astype(np.int32)
            if not c.any() or not r.any():
                continue
            for cyc in (True, False):
                got = s1.flag_windows(r, c, cyc)
                assert got == C.windows_ref(r, c, cyc), (r, c, cyc)
                assert all(type(g) is int for g in got)
                j0, nj_sel, i0, ni_sel = got                       # every flagged row and column lies in the window
                assert set(np.nonzero(c)[0]) <= set((i0 + np.arange(ni_sel)) % ni) and 1 <= ni_sel <= ni and 0 <= i0 < ni
                assert set(np.nonzero(r)[0]) <= set(range(j0, j0 + nj_sel))
                n += 1
    assert n > 300
    with pytest.raises(ValueError, match='no row or column'):
        s1.flag_windows(np.zeros(3, dtype=np.int32), np.ones(4, dtype=np.int32), True)


# ------------------------------------------------------------------------------- 3. the auto detection
@pytest.mark.parametrize('shape', C.AUTO_SHAPES)
def test_auto_detection(s1, shape):
    for name, (lat, lon, want) in C.grid_kinds(*shape).items():
        assert C.cyclic_ref(lat, lon) is want, (shape, name)
        assert s1.grid_is_cyclic(lat, lon) is want, (shape, name)
        assert s1.grid_is_cyclic(lat.astype(np.float32), lon.astype(np.float32)) is want
    lat, lon = C.regional_grid()
    assert s1.grid_is_cyclic(lat, lon) is False and C.cyclic_ref(lat, lon) is False


def test_auto_detection_edges(s1):
    lat, lon = C.ocean_grid(12, 65)
    assert s1.grid_is_cyclic(lat[:, :2], lon[:, :2]) is False                  # ni < 3
    bad = lon.copy()
    bad[:, 0] = np.nan                                                         # no row with four finite end cells
    assert s1.grid_is_cyclic(lat, bad) is False and C.cyclic_ref(lat, bad) is False
    some = lon.copy()
    some[:5, -1] = np.inf                                                      # the other rows decide
    assert s1.grid_is_cyclic(lat, some) is True and C.cyclic_ref(lat, some) is True
    assert s1.grid_is_cyclic(lat[:, :3], lon[:, :3]) is C.cyclic_ref(lat[:, :3], lon[:, :3])


# ------------------------------------------------------------------------------- 4. the cases carry their own conditions
def test_seam_case_condition():
    lat, lon = C.ocean_grid(40, 60)
    j0, nj_sel, i0, ni_sel, n = C.box_ref(lat, lon, C.REF_BOX, cyclic=True)
    assert n >= 2 and ni_sel <= 60 / 2 and ni_sel == 19 and i0 + ni_sel > 60       # the window wraps
    assert C.box_ref(lat, lon, C.REF_BOX, cyclic=False)[2:4] == (0, 60)
    assert C.box_ref(lat, lon, C.REF_BOX, cyclic='auto') == (j0, nj_sel, i0, ni_sel, n)
    for name, (la, lo, cyc) in C.grid_kinds(40, 60).items():                       # every kind, every box: a real selection
        for box in C.BOXES:
            got = C.box_ref(la, lo, box)
            assert got[4] >= 2, (name, box)
    assert C.box_ref(lat, lon, C.ASIA_BOX)[3] < 60 and C.box_ref(lat, lon, C.ASIA_BOX)[1] < 40
    la, lo = C.regional_grid()
    got = C.box_ref(la, lo, (10.0, 30.0, 35.0, 50.0))
    assert got[4] >= 2 and got[1] < la.shape[0] and got[3] < la.shape[1]
    # the other grids the GPU tests cut: the halo grid across its seam, and the source of the chain into step_02
    la, lo, cyc = C.grid_kinds(12, 65)['halo']
    got = C.box_ref(la, lo, C.REF_BOX)
    assert cyc and got[4] >= 2 and got[2] + got[3] > la.shape[1] and got[3] <= la.shape[1] / 2
    la, lo = C.ocean_grid(90, 180)
    got = C.box_ref(la, lo, C.ASIA_BOX)
    assert got[4] >= 2 and got[1] < 90 and got[3] < 180 / 2


@pytest.mark.parametrize('dtype', [np.float64, np.float32])
def test_edge_case_condition(dtype):
    lat, lon, table = C.edge_grid(dtype)
    assert lat.dtype == dtype and lon.dtype == dtype
    ins = C.inside_ref(lat, lon, C.REF_BOX).reshape(-1)
    want = C.edge_expectation(table)
    for n, edge, kind in table:
        assert bool(ins[n]) is want[n], (n, edge, kind, lat.reshape(-1)[n], lon.reshape(-1)[n])
    assert ins.sum() == sum(want.values()) >= 2                    # nothing else of the grid is inside
    lon1, lon2, lat1, lat2 = C.REF_BOX
    fl, fo = lat.reshape(-1).astype(np.float64), lon.reshape(-1).astype(np.float64)
    for edge, value in (('lat_lo', lat1), ('lat_hi', lat2)):
        on = [n for n, e, k in table if e == edge and k == 'on']
        out = [n for n, e, k in table if e == edge and k == 'out']
        assert len(on) >= 1 and all(fl[n] == value for n in on) and len(out) >= 1
        for n in out:                                              # exactly one ulp of the dtype away, on the far side
            assert abs(fl[n]) > abs(value) and np.nextafter(lat.reshape(-1)[n], dtype(0)) == dtype(value)
    for edge, value in (('lon1', lon1), ('lon2', lon2)):
        on = [n for n, e, k in table if e == edge and k == 'on']
        out = [n for n, e, k in table if e == edge and k == 'out']
        assert sorted(fo[n] - value for n in on) == [-360.0, 0.0, 360.0]            # k = +1, 0, -1
        assert len(out) == 3
        for n, m in zip(on, out):
            toward = dtype(-np.inf) if edge == 'lon1' else dtype(np.inf)
            assert lon.reshape(-1)[m] == np.nextafter(lon.reshape(-1)[n], toward)
    assert {287.0, 397.0} <= set(fo.tolist())


# ------------------------------------------------------------------------------- 5. errors before the device is touched
def test_errors_before_the_device(s1, no_device, tmp_path):
    lat, lon = C.ocean_grid(8, 12)
    for box in ((10, 5, 0, 1), (0, 361, 0, 1), (5, 5, 0, 1), (0, 1, 2), 'abc', (np.nan, 5, 0, 1), (0, 5, np.nan, 1)):
        with pytest.raises(ValueError, match='box'):
            s1.curvilinear_box(lat, lon, box)
    with pytest.raises(ValueError, match='2-D arrays of one shape'):
        s1.curvilinear_box(lat, lon[:, :-1], C.REF_BOX)
    with pytest.raises(ValueError, match='2-D arrays of one shape'):
        s1.curvilinear_box(lat[0], lon[0], C.REF_BOX)
    with pytest.raises(ValueError, match='cyclic'):
        s1.curvilinear_box(lat, lon, C.REF_BOX, cyclic='maybe')
    data = np.zeros((2, 8, 12), dtype=np.float32)
    with pytest.raises(ValueError, match='do not match the last two axes'):
        s1.select(data, box=C.REF_BOX, lat=lat[:, :-1], lon=lon[:, :-1])
    with pytest.raises(ValueError, match='do not match the last two axes'):
        s1.select(data[:, :7], box=C.REF_BOX, lat=lat, lon=lon)
    with pytest.raises(ValueError, match='box'):
        s1.select(data, box=(10, 5, 0, 1), lat=lat, lon=lon)
    # 1-D coordinates: lonlat_box is as it was, and cyclic must stay 'auto'
    with pytest.raises(ValueError, match='not supported here'):
        s1.lonlat_box(lat, lon, C.REF_BOX)
    lat1, lon1 = np.linspace(-70, 70, 8), np.arange(0.0, 360.0, 30.0)
    with pytest.raises(ValueError, match='cyclic'):
        s1.select(data, box=C.REF_BOX, lat=lat1, lon=lon1, cyclic=True)
    import test_step01_select_hip as T
    values, vattrs = T.case_values('f4_fill')
    inp = T.write_file(str(tmp_path / 'in.nc'), 'ta', values, [15.5, 45.0, 74.5], vattrs)
    for argv in (['select', '-i', inp, '-o', str(tmp_path / 'o.nc'), '-v', 'ta', '-b', '-73,37,-42,34', '--cyclic', 'yes'],
                 ['climatology', '-i', inp, '-o', str(tmp_path / 'o.nc'), '-v', 'ta', '-m', 'ymonmean', '-b', '-73,37,-42,34',
                  '--cyclic', 'no']):
        with pytest.raises(ValueError, match='cyclic'):
            s1.main(argv)
    with pytest.raises(SystemExit):
        s1.main(['select', '-i', inp, '-o', str(tmp_path / 'o.nc'), '-v', 'ta', '-b', '-73,37,-42,34', '--cyclic', 'maybe'])
