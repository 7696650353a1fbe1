"""Cases of tests/test_source_points_hip.py and tests/test_source_points_host.py: step_03 on climate deltas that lie on the
GCM's grid with every column of the ERA5 file a target of its own (settings.delta_grid = 'source_points'), the winds rotated
onto a rotated-pole file's directions (--rotate_winds), and the points plan behind it (pgw_points_plan_create / _apply /
_apply_wind / _destroy).

Everything here is host code.  The reference of every comparison is code that was there before: `functions.regrid_points` /
`regrid_points_wind` / `regrid_lat_lon_wind` (pgw_regrid_points, pgw_regrid_points_wind) on the whole array with the cast made
on the host, `RegridPlan.apply` for a mesh handed over as points, and for the runs `step_02 regridding [--rotate_winds]` into
files with step_03 on them, or `--delta_grid source` on mesh files - never the points plan or the paired provider themselves.
All comparisons are for equal bits or bytes, so no tolerance is derived.  `conditions()` asserts on the CPU what the cases
exist for."""
import numpy as np

import points_file_cases as P
import source_delta_cases as K
import wind_rotation_cases as W

BLOCK = 256                                  # threads per block of k_regrid_points / k_regrid_points_wind: one target per lane
WAVE = 64
NPOINTS = W.NPOINTS                          # 1, 63, 64, 65: around a wave; 257, 513: two and three blocks, the last ragged
NFIELDS = K.NFIELDS                          # applies on one plan, in this order: max_nfield first, then fewer planes
OFFSETS = K.OFFSETS
GUARD = K.GUARD
FILES = P.FILES


def pole_of(i):
    """The rotated pole of the i-th case: every pole of wind_rotation_cases.POLES comes round."""
    return W.POLES[i % len(W.POLES)]


def targets(pair, n):
    """n point-wise targets for a grid pair of source_delta_cases.grid_pairs(): in random order inside the box the pair's
    mesh target spans (so the source covers them), the first two - where there are that many - on the box's lowest and
    highest latitude: with a `poles` pair these are the poles themselves, and the targets beyond the source's last rows
    bracket a pole row."""
    name, _, _, tlat, tlon = pair
    rng = np.random.default_rng(n + len(name))
    lat = rng.uniform(tlat.min(), tlat.max(), n)
    lon = rng.uniform(tlon.min(), tlon.max(), n)
    if n >= 2:
        lat[0], lat[1] = tlat.min(), tlat.max()
    return lat, lon


def point_tables(pair, lat, lon):
    """regrid_tables of the ravelled targets with the `oob` table of the point-wise entries."""
    from pgw4era5_amd import functions as F
    tb = F.regrid_tables(pair[1], pair[2], np.ravel(lat), np.ravel(lon))
    tb['oob'] = np.ascontiguousarray(tb['lat_oob'] | tb['lon_oob'], dtype=np.int32)
    return tb


def flagged(tb, n):
    """The tables with every third target flagged oob and its entries made unreadable (rows and columns far outside): what
    regrid_tables never hands out - it raises the extent error instead - and the C entries must still serve."""
    t = {k: (np.array(v, copy=True) if isinstance(v, np.ndarray) else v) for k, v in tb.items()}
    idx = np.arange(0, n, 3)
    t['oob'][idx] = 1
    for k in ('lat_lo', 'lat_hi', 'lon_lo', 'lon_hi'):
        t[k][idx] = 1 << 20
    return t, idx


def conditions():
    """What the shapes exist for, as counts on the CPU -> dict of the counts."""
    cols = P.conditions()
    assert cols['rotated 7x9'] == 63 and cols['rotated 7x9'] < WAVE                         # below a wave
    assert cols['rotated 11x24'] == 264 and BLOCK < 264 < 2 * BLOCK and 264 % BLOCK != 0    # two blocks, the last ragged
    assert cols['cells 65'] == 65 and not np.array_equal(P.PERM, np.arange(65))              # a permuted cell list
    assert NPOINTS == [1, 63, 64, 65, 257, 513] and max(NFIELDS) == NFIELDS[0]
    assert [-(-n // BLOCK) for n in NPOINTS] == [1, 1, 1, 1, 2, 3] and all(n % BLOCK for n in NPOINTS)
    n_pole = n_nan = n_oob = n_pairs = 0
    poles_seen = set()
    for i, pair in enumerate(K.grid_pairs()):
        n_pairs += 1
        for j, n in enumerate(NPOINTS):
            poles_seen.add(pole_of(i + j))
            lat, lon = targets(pair, n)
            tb = point_tables(pair, lat, lon)
            assert not tb['oob'].any()                       # regrid_tables raises for what it does not cover
            nlat_s = len(pair[1])
            pole_rows = ((tb['lat_lo'] == -1) | (tb['lat_hi'] == -1) | (tb['lat_lo'] == nlat_s) | (tb['lat_hi'] == nlat_s))
            if pair[0].endswith('poles') and n >= 2:
                assert pole_rows[:2].all() and tb['south_row'] >= 0 and tb['north_row'] >= 0
            elif not pair[0].endswith('poles'):
                assert not pole_rows.any()
            n_pole += int(pole_rows.sum())
            # targets one of whose four corners is NaN in the first plane of plan_field(nan=tb)
            f = K.plan_field(pair[0], 3, nlat_s, len(pair[2]), np.float64, nan=tb)[0]
            rows = lambda r: np.clip(r, 0, nlat_s - 1)
            corner = np.zeros(n, dtype=bool)
            for r in ('lat_lo', 'lat_hi'):
                for c in ('lon_lo', 'lon_hi'):
                    inside = (tb[r] >= 0) & (tb[r] < nlat_s)
                    corner |= inside & np.isnan(f[rows(tb[r]), tb[c]])
            assert corner.any(), (pair[0], n)
            n_nan += int(corner.sum())
            n_oob += len(flagged(tb, n)[1])
    assert n_pairs == len(K.grid_pairs()) and poles_seen == set(W.POLES)
    assert n_pole > 0 and n_nan > 0 and n_oob > 0
    assert K.conditions()                                    # the walks of the record tests are source_delta_cases'
    return dict(pole=n_pole, nan=n_nan, oob=n_oob)
