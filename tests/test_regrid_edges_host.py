"""The lat-lon regridding (`pgw_regrid_bilinear`: k_regrid, k_zonal_mean_rows; host tables `functions.regrid_tables`) at
its window, slice and pole edges: the references, the case builders and the host tests that keep both honest.  The GPU
tests of tests/test_regrid_edges_hip.py import everything from here.  No GPU is needed in this file.

`regrid_reference` restates the reference's xarray branch (functions.py:774-789, 817-893) from the coordinates alone, in
np.longdouble: flip, pole rows (NaN-skipping zonal mean, all NaN gives NaN), +-360 copies, scipy's index rule
(searchsorted-left, clip to [1, n - 1]) and slope * (x_new - x_lo) + y_lo.  Every decision (which neighbours, in or out
of bounds) is taken on the float64 coordinates the reference itself forms; only the arithmetic on values is wider.

`kernel_statement` restates k_regrid in float64 from the `regrid_tables` output: the same IEEE operations in the same
order, the pole values supplied from outside.

The bound that comes with the reference (`regrid_reference(...)[1]`, per output value), derived, not tuned.  eps = 2^-52.
  one interpolation   fl(fl(fl(y_hi - y_lo) / fl(x_hi - x_lo)) * fl(x_new - x_lo)) + y_lo, the last sum rounded too: five
                      roundings on the term, whose size is at most |y_hi - y_lo| (0 <= x_new - x_lo <= x_hi - x_lo in
                      bounds), and one on the result, at most max(|y_lo|, |y_hi|): below 6 (eps / 2) (|y_lo| + |y_hi|) to
                      first order; taken as 4 eps (|y_lo| + |y_hi|).  Errors e_lo, e_hi that the two neighbours already
                      carry come through with weights 1 - w and w in [0, 1]: at most e_lo + e_hi.
  pole row            the mean of the n valid values of a source row, summed in ANY order, is off by at most
                      (n - 1) eps sum|v| / n, and the quotient adds one rounding, eps |mean|: this is the error a pole
                      row carries into the latitude pass, and through it with a weight of at most 1 into the longitude
                      pass - per target e_pole <= (n - 1) eps (sum|v| / n) + eps |mean| on top of the two interpolations.
                      Source rows carry none.
  float32 storage     the float32 inputs widen exactly, so the bound above holds on them as it stands; the one rounding of
                      the result to float32 adds 2^-24 |ref|.
The oracle (oracle.pgw_oracle.regrid_lat_lon) and the kernel perform these float64 operations (the kernel with
-ffp-contract=off and SharedDivisor's correctly rounded quotient), so both are held to this bound; where no pole row is
in a target's stencil the kernel is in addition held to the BITS of `kernel_statement`.  NaN masks are compared exactly.

Every case builder asserts the condition that makes its case an edge (from `block_spans` and `slices`, which restate the
kernel's window rule and the launch rule of pgw_regrid_bilinear), so a later change to a helper or to the launch rule
fails the case's own condition instead of silently turning it into an ordinary case."""
import functools

import numpy as np
import pytest

from oracle import pgw_oracle as O
from pgw4era5_amd.functions import regrid_tables

EPS = float(np.finfo(np.float64).eps)
LD = np.longdouble
BLOCK = 256                        # threads per block of k_regrid
REGRID_SPAN = 256                  # source columns a block can stage in LDS
FU = 4                             # planes per step of a block's walk through its z-slice
WORST = {}                         # group -> largest observed error / bound


def record(name, err, bound):
    pos = bound > 0
    if pos.any():
        WORST[name] = max(WORST.get(name, 0.0), float((err[pos] / bound[pos]).max()))


# ------------------------------------------------------------------ the reference, from the coordinates
def _zonal_mean_ld(row):
    """NaN-skipping mean over the last axis in longdouble; all NaN gives NaN.  Returns (mean, error a float64 mean summed in
    any order may carry)."""
    ok = ~np.isnan(row)
    n = ok.sum(axis=-1)
    v = np.where(ok, row, LD(0))
    with np.errstate(invalid='ignore', divide='ignore'):
        mean = np.where(n > 0, v.sum(axis=-1) / np.maximum(n, 1), LD(np.nan))
        err = np.where(n > 0, (n - 1) * LD(EPS) * (np.abs(v).sum(axis=-1) / np.maximum(n, 1)) + LD(EPS) * np.abs(mean), LD(np.nan))
    return mean, err


def _interp_ld(x, y, e, x_new, axis):
    """scipy interp1d(kind='linear', bounds_error=False, assume_sorted=False) on longdouble values y that carry the errors e."""
    y, e = np.moveaxis(y, axis, 0), np.moveaxis(e, axis, 0)
    if np.any(np.diff(x) < 0):                                    # xarray sorts by coordinate before interpolating
        order = np.argsort(x, kind='stable')
        x, y, e = x[order], y[order], e[order]
    idx = np.searchsorted(x, x_new).clip(1, len(x) - 1).astype(int)
    shp = (-1,) + (1,) * (y.ndim - 1)
    x_lo, x_hi = x[idx - 1].astype(LD).reshape(shp), x[idx].astype(LD).reshape(shp)
    y_lo, y_hi = y[idx - 1], y[idx]
    with np.errstate(invalid='ignore', divide='ignore'):
        slope = (y_hi - y_lo) / (x_hi - x_lo)
        y_new = slope * (x_new.astype(LD).reshape(shp) - x_lo) + y_lo
    e_new = e[idx - 1] + e[idx] + 4 * LD(EPS) * (np.abs(y_lo) + np.abs(y_hi))
    y_new[(x_new < x[0]) | (x_new > x[-1])] = np.nan
    e_new = np.where(np.isnan(y_new), LD(np.nan), e_new)
    return np.moveaxis(y_new, 0, axis), np.moveaxis(e_new, 0, axis)


def regrid_reference(field, src_lat, src_lon, targ_lat, targ_lon):
    """field (..., nlat_s, nlon_s) float32 / float64 -> (out, bound), both (..., nlat_t, nlon_t) longdouble; `bound` is the
    error a float64 evaluation of the same formula may have (module docstring), NaN where `out` is."""
    f = np.asarray(field).astype(LD)
    lat, lon, tlat, tlon = (np.asarray(a, dtype=np.float64) for a in (src_lat, src_lon, targ_lat, targ_lon))
    e = np.zeros(f.shape, dtype=LD)
    dlon = np.median(np.diff(lon))                                # :778
    dlat = np.median(np.diff(lat))                                # :779, before the flip
    periodic = (dlon + np.max(lon) - np.min(lon)) >= 359.9        # :780-789
    if lat[0] > lat[-1]:                                          # :822-829
        lat, f, e = lat[::-1], f[..., ::-1, :], e[..., ::-1, :]

    def pole_row(row):
        m, me = _zonal_mean_ld(row)
        return (np.broadcast_to(m[..., None, None], row[..., None, :].shape),
                np.broadcast_to(me[..., None, None], row[..., None, :].shape))
    if np.max(tlat) + dlat > 89.9:                                # :833-837
        p, pe = pole_row(f[..., -1, :])
        f, e, lat = np.concatenate([f, p], axis=-2), np.concatenate([e, pe], axis=-2), np.concatenate([lat, [90.0]])
    if np.min(tlat) - dlat < -89.9:                               # :838-842
        p, pe = pole_row(f[..., 0, :])
        f, e, lat = np.concatenate([p, f], axis=-2), np.concatenate([pe, e], axis=-2), np.concatenate([[-90.0], lat])
    if (np.max(tlat) > np.max(lat)) | (np.min(tlat) < np.min(lat)):          # :845-856
        raise ValueError('ERA5 dataset extends further North or South than GCM dataset!')
    f, e = _interp_ld(lat, f, e, tlat, -2)                        # :859
    if periodic:                                                  # :866-874
        if np.max(tlon) > np.max(lon):
            f, e, lon = np.concatenate([f, f], axis=-1), np.concatenate([e, e], axis=-1), np.concatenate([lon, lon + 360])
        if np.min(tlon) < np.min(lon):                            # the (possibly already extended) dataset, shifted
            f, e, lon = np.concatenate([f, f], axis=-1), np.concatenate([e, e], axis=-1), np.concatenate([lon - 360, lon])
    if (np.max(tlon) > np.max(lon)) | (np.min(tlon) < np.min(lon)):          # :877-888
        raise ValueError('ERA5 dataset extends further East or West than GCM dataset!')
    return _interp_ld(lon, f, e, tlon, -1)                        # :892


# ------------------------------------------------------------------ the kernel, in numpy
def _div(n, d):
    """SharedDivisor(d).divide(n): the correctly rounded quotient; a zero divisor gives NaN (its reciprocal is not finite)."""
    with np.errstate(invalid='ignore', divide='ignore'):
        return np.where(d == 0, np.nan, n / np.where(d == 0, 1.0, d))


def kernel_statement(field, tb, pole=None):
    """k_regrid on tables `tb` (regrid_tables' keys) in float64: per plane the latitude pass at every source column, then
    the longitude pass between two of them; `pole` (nfield, 2): the south / north pole value of each plane (None: no
    table entry may name a pole row).  Returns (nfield, nlat_t, nlon_t) of the field's dtype."""
    field = np.asarray(field)
    nlat_s, nlon_s = field.shape[-2:]
    f = field.reshape(-1, nlat_s, nlon_s).astype(np.float64)
    nlat_t, nlon_t = len(tb['lat_lo']), len(tb['lon_lo'])
    out = np.empty((f.shape[0], nlat_t, nlon_t))

    def row(r):
        if 0 <= r < nlat_s:
            return f[:, r, :]
        return np.repeat(pole[:, 0 if r < 0 else 1, None], nlon_s, axis=1)
    il, ih = tb['lon_lo'], tb['lon_hi']
    with np.errstate(invalid='ignore'):
        for j in range(nlat_t):
            if tb['lat_oob'][j]:
                out[:, j, :] = np.nan
                continue
            lo, hi = row(tb['lat_lo'][j]), row(tb['lat_hi'][j])
            y = _div(hi - lo, tb['lat_Dx'][j]) * tb['lat_dx'][j] + lo          # lat pass, :859
            ya, yb = y[:, il], y[:, ih]
            out[:, j, :] = _div(yb - ya, tb['lon_Dx'][None, :]) * tb['lon_dx'][None, :] + ya        # lon pass, :892
    out[:, :, tb['lon_oob'] != 0] = np.nan
    return out.astype(field.dtype)


def pole_rows(tb, nlat_s):
    """(nlat_t,) bool: target rows whose stencil holds a pole row."""
    return (tb['lat_lo'] < 0) | (tb['lat_lo'] >= nlat_s) | (tb['lat_hi'] < 0) | (tb['lat_hi'] >= nlat_s)


# ------------------------------------------------------------------ the kernel's window rule and the launch rule
def launch_w(nlon_t, force_vec1=False):
    """Target longitudes per thread (the output of a device allocation is aligned)."""
    return 2 if (nlon_t % 2 == 0 and not force_vec1) else 1


def block_spans(tb, nlon_s, nlon_t, W):
    """[(c0, span, first)] per block of BLOCK * W consecutive target longitudes, as k_regrid forms them: c0 = lon_lo of
    the first valid (not lon_oob) target, offsets of every valid target's two neighbours from c0 modulo nlon_s, span =
    the largest + 1.  A block without a valid target: (0, 0, BLOCK * W)."""
    res = []
    for b0 in range(0, nlon_t, BLOCK * W):
        i = np.arange(b0, min(b0 + BLOCK * W, nlon_t))
        valid = tb['lon_oob'][i] == 0
        if not valid.any():
            res.append((0, 0, BLOCK * W))
            continue
        first = int(np.flatnonzero(valid)[0])
        c0 = int(tb['lon_lo'][b0 + first])
        rl = (tb['lon_lo'][i][valid].astype(np.int64) - c0) % nlon_s
        rh = (tb['lon_hi'][i][valid].astype(np.int64) - c0) % nlon_s
        res.append((c0, int(max(rl.max(), rh.max())) + 1, first))
    return res


def staged(span):
    return span <= REGRID_SPAN


def slices(nfield, nlat_t, nlon_t, W):
    """The launch rule of pgw_regrid_bilinear: dict(bx, gz, per, sizes) - blocks per target row, z-slices, planes per
    slice and the planes each slice really has (0: an empty slice)."""
    bx = -(-nlon_t // (BLOCK * W))
    xy = bx * nlat_t
    want = -(-8192 // xy)
    gz = min(max(want, 1), nfield)
    if nfield >= 8:
        gz = -(-gz // 8) * 8
    gz = min(gz, nfield)
    per = -(-nfield // gz)
    sizes = [max(0, min(nfield, (z + 1) * per) - z * per) for z in range(gz)]
    assert sum(sizes) == nfield
    return dict(bx=bx, gz=gz, per=per, sizes=sizes)


# ------------------------------------------------------------------ the cases
class Case:
    """Inputs of one regridding call: field (float64; cast by the GPU tests), the four coordinate vectors, force_vec1."""

    def __init__(self, field, src_lat, src_lon, targ_lat, targ_lon, force_vec1=False):
        self.field = np.ascontiguousarray(field, dtype=np.float64)
        self.src_lat, self.src_lon, self.targ_lat, self.targ_lon = (
            np.ascontiguousarray(a, dtype=np.float64) for a in (src_lat, src_lon, targ_lat, targ_lon))
        self.force_vec1 = force_vec1
        self.nlat_s, self.nlon_s, self.nlat_t, self.nlon_t = len(src_lat), len(src_lon), len(targ_lat), len(targ_lon)
        assert self.field.shape[-2:] == (self.nlat_s, self.nlon_s)
        self.nfield = int(np.prod(self.field.shape[:-2], dtype=np.int64))
        self.tb = regrid_tables(self.src_lat, self.src_lon, self.targ_lat, self.targ_lon)
        self.W = launch_w(self.nlon_t, force_vec1)
        self.spans = block_spans(self.tb, self.nlon_s, self.nlon_t, self.W)
        self.slices = slices(self.nfield, self.nlat_t, self.nlon_t, self.W)
        self.pole_rows = pole_rows(self.tb, self.nlat_s)
        self._ref = {}

    def typed(self, dtype):
        return self.field.astype(dtype)

    def reference(self, dtype=np.float64):
        """(ref, bound) of the field as stored in `dtype`, computed once."""
        key = np.dtype(dtype).name
        if key not in self._ref:
            ref, bound = regrid_reference(self.typed(dtype), self.src_lat, self.src_lon, self.targ_lat, self.targ_lon)
            if key == 'float32':
                bound = bound + LD(2.0 ** -24) * np.abs(ref)
            self._ref[key] = (ref, bound)
        return self._ref[key]

    def numpy_poles(self, dtype=np.float64):
        """(nfield, 2) pole values for kernel_statement, numpy's own nanmean: only for the NaN mask and the rows away
        from the poles, whose bits do not depend on them."""
        f = self.typed(dtype).reshape(-1, self.nlat_s, self.nlon_s).astype(np.float64)
        p = np.full((self.nfield, 2), np.nan)
        for k, r in enumerate((self.tb['south_row'], self.tb['north_row'])):
            if r >= 0:
                p[:, k] = O._zonal_mean(f[:, r, :])
        return p


def _field(rng, shape, planes_distinct=True):
    """Values of both signs, never 0; plane k lies around 100 (k + 1), so a plane taken from the wrong source plane shows."""
    f = rng.normal(0.0, 5.0, shape)
    if planes_distinct:
        f = f + 100.0 * (1 + np.arange(int(np.prod(shape[:-2]))).reshape(shape[:-2] + (1, 1)))
    return f


LATS24 = np.linspace(-87.5, 87.5, 24) + 0.3 * np.sin(np.arange(24))          # ascending, short of both poles, uneven
TLATS5 = np.array([-90.0, -88.9, 0.3, 88.2, 90.0])                            # both pole rows, rows next to them, one inside


def _window_case(nlon_s, nlon_t=1536, force_vec1=False, shift=0.0):
    rng = np.random.default_rng(nlon_s * 7 + nlon_t)
    tlon = (np.arange(1536) * (360.0 / 1536))[:nlon_t] + shift
    return Case(_field(rng, (3, 24, nlon_s)), LATS24, np.arange(nlon_s) * (360.0 / nlon_s), TLATS5, tlon, force_vec1)


def case_window_765():
    """One staged block (span 256) and two direct ones (257) in one launch."""
    c = _window_case(765)
    assert c.W == 2 and [s for _, s, _ in c.spans] == [256, 257, 257] and c.tb['periodic']
    return c


def case_window_768():
    c = _window_case(768)
    assert c.W == 2 and len(c.spans) == 3 and all(s > REGRID_SPAN for _, s, _ in c.spans)
    return c


def case_window_765_vec1():
    c = _window_case(765, force_vec1=True)
    assert c.W == 1 and len(c.spans) == 6 and all(129 <= s <= 130 for _, s, _ in c.spans)
    return c


def case_window_765_odd():
    c = _window_case(765, nlon_t=1535)
    assert c.W == 1 and len(c.spans) == 6 and all(s <= REGRID_SPAN for _, s, _ in c.spans)
    return c


def _gap_and_seam(c):
    """(a block starts in the periodic gap, a staged block's window runs over the seam)"""
    return (any(s > 0 and c0 == c.nlon_s - 1 for c0, s, _ in c.spans),
            any(0 < s <= REGRID_SPAN and c0 + s > c.nlon_s for c0, s, _ in c.spans))


# target 512 of the shifted axis lies at 120 + shift: in the gap (359.53, 360) of the 765-column source
SHIFT_GAP = 239.8


def case_seam_gap_w2():
    """W = 2: block 1 starts in the gap."""
    c = _window_case(765, shift=SHIFT_GAP)
    assert c.W == 2 and c.src_lon[-1] < c.targ_lon[512] < 360.0 and c.targ_lon.max() > 360.0
    assert _gap_and_seam(c)[0]
    return c


def case_seam_gap_w1():
    """W = 1: block 2 starts in the gap and is staged, so its window runs over the seam."""
    c = _window_case(765, force_vec1=True, shift=SHIFT_GAP)
    assert c.W == 1 and _gap_and_seam(c) == (True, True)
    assert any(c0 == c.nlon_s - 1 and staged(s) for c0, s, _ in c.spans)
    return c


def case_seam_mid_block():
    """The seam in the middle of a staged block (W = 1: every block is staged)."""
    c = _window_case(765, force_vec1=True, shift=330.0)
    hit = [(c0, s) for c0, s, _ in c.spans if staged(s) and c0 + s > c.nlon_s]
    assert c.W == 1 and hit and all(c0 < c.nlon_s - 40 for c0, s in hit)          # the seam is well inside the window
    return c


def case_seam_staged_w2():
    """W = 2 and a staged block over the seam: 720 source columns, windows of 241 to 242."""
    rng = np.random.default_rng(720)
    tlon = np.arange(1536) * (360.0 / 1536) + 300.0
    c = Case(_field(rng, (2, 24, 720)), LATS24, np.arange(720) * 0.5, TLATS5, tlon)
    assert c.W == 2 and _gap_and_seam(c)[1] and all(staged(s) for _, s, _ in c.spans)
    return c


def _slice_case(nfield, nlat_t):
    rng = np.random.default_rng(nfield)
    shape = (6, 12) if nfield == 1 else (nfield, 6, 12)           # 1: a 2-D field
    slat = np.array([-75.0, -40.0, -10.0, 15.0, 50.0, 80.0])
    tlat = np.linspace(-74.0, 79.0, nlat_t)                        # interior: no pole row, every value's bits are pinned
    c = Case(_field(rng, shape), slat, np.arange(12) * 30.0, tlat, np.arange(8) * 45.0 + 3.0)
    assert c.W == 2 and c.slices['bx'] == 1 and not c.pole_rows.any() and c.nfield == nfield
    return c


def case_slices(nfield):
    c = _slice_case(nfield, 5 if nfield <= 16 else 1100)
    s = c.slices
    if nfield == 1:
        assert c.field.ndim == 2 and s['gz'] == 1
    elif nfield in (7, 9):
        assert s['gz'] == nfield and s['gz'] % 8 != 0 and s['per'] == 1
    elif nfield in (8, 16):
        assert s['gz'] == nfield and s['gz'] % 8 == 0 and s['per'] == 1
    elif nfield == 19:                                             # ragged slice shorter than FU, and an empty one
        assert s['gz'] == 8 and s['per'] == 3 and s['sizes'] == [3, 3, 3, 3, 3, 3, 1, 0]
    elif nfield == 40:                                             # a full step of FU planes and a ragged one
        assert s['gz'] == 8 and s['per'] == 5 and s['per'] > FU and s['per'] % FU != 0
    else:
        raise KeyError(nfield)
    return c


SLAT12 = np.linspace(-82.0, 82.0, 12) + 0.5 * np.cos(np.arange(12))
SLON70 = np.arange(70) * (360.0 / 70)                               # more than one wave's stride, not a multiple of 64
TLON9 = np.array([0.0, 3.3, 77.7, 180.0, 200.1, 354.86, 355.0, 359.0, 359.9])


def _pole_field(rng, nlat_s=12, nlon_s=70):
    """Plane 0 clean; plane 1: both edge rows partly NaN; plane 2: both edge rows all NaN; plane 3 clean."""
    f = _field(rng, (4, nlat_s, nlon_s))
    for r in (0, nlat_s - 1):
        f[1, r, [0, 5, 63, 64, nlon_s - 1]] = np.nan
        f[2, r, :] = np.nan
    return f


def case_pole_south_only():
    c = Case(_pole_field(np.random.default_rng(41)), SLAT12, SLON70, np.array([-90.0, -89.0, -84.0, -80.0, -30.0, 0.0]), TLON9)
    assert c.tb['south_row'] == 0 and c.tb['north_row'] == -1 and c.pole_rows.tolist() == [True, True, True, False, False, False]
    return c


def case_pole_north_only():
    c = Case(_pole_field(np.random.default_rng(42)), SLAT12, SLON70, np.array([0.0, 30.0, 80.0, 84.0, 89.0, 90.0]), TLON9)
    assert c.tb['south_row'] == -1 and c.tb['north_row'] == 11 and c.pole_rows.tolist() == [False, False, False, True, True, True]
    return c


def case_pole_none():
    c = Case(_pole_field(np.random.default_rng(43)), SLAT12, SLON70, np.array([-60.0, -30.0, 0.0, 30.0, 60.0]), TLON9)
    assert c.tb['south_row'] == c.tb['north_row'] == -1 and not c.pole_rows.any()
    return c


def case_pole_in_source():
    """Source latitudes that include -90 and 90 under a global target: the reference's pole row at -90 lies next to the
    source's own, x_hi - x_lo = 0, and exactly the target row at -90 is NaN (at 90 searchsorted-left finds the source's)."""
    slat = np.linspace(-90.0, 90.0, 13)
    tlat = np.array([-90.0, -89.5, -75.0, 0.0, 75.0, 89.5, 90.0])
    c = Case(_field(np.random.default_rng(44), (3, 13, 70)), slat, SLON70, tlat, TLON9)
    assert c.tb['south_row'] == 0 and c.tb['north_row'] == 12
    assert c.tb['lat_Dx'][0] == 0.0 and (c.tb['lat_Dx'][1:] > 0).all()
    assert (c.tb['lat_lo'][0], c.tb['lat_hi'][0]) == (-1, 0) and not c.pole_rows[1:].any()
    ref, _ = c.reference()
    assert np.isnan(ref[:, 0, :]).all() and not np.isnan(ref[:, 1:, :]).any()
    return c


def case_descending_source():
    """Descending source latitudes (dlat < 0: no pole rows) with interior targets: the rows come back un-flipped."""
    c = Case(_field(np.random.default_rng(51), (3, 12, 70)), SLAT12[::-1], SLON70, np.array([-70.0, -1.0, 33.3, 71.0]), TLON9)
    assert (c.tb['lat_lo'] > c.tb['lat_hi']).all() and not c.pole_rows.any()
    return c


def case_descending_targets():
    c = Case(_field(np.random.default_rng(52), (3, 12, 70)), SLAT12, SLON70, TLATS5[::-1].copy(), TLON9[::-1].copy())
    assert (np.diff(c.targ_lat) < 0).all() and (np.diff(c.targ_lon) < 0).all() and c.pole_rows.sum() == 4
    return c


def case_descending_both():
    c = Case(_field(np.random.default_rng(53), (2, 12, 70)), SLAT12[::-1], SLON70, np.array([71.0, 33.3, -1.0, -70.0]), TLON9)
    assert (c.tb['lat_lo'] > c.tb['lat_hi']).all() and (np.diff(c.targ_lat) < 0).all()
    return c


def case_unsorted_duplicate_targets():
    rng = np.random.default_rng(54)
    tlat = np.array([10.0, -90.0, 88.8, 10.0, -45.5, 90.0, -45.5, 0.0])
    # one block of shuffled targets with duplicates among them, then 49 ascending ones: a direct and a staged block
    tlon = np.concatenate([rng.permutation(np.arange(251) * 1.4), [0.0, 0.0, 123.6, 123.6, 358.8], 200.0 + np.arange(49) * 1.2])
    c = Case(_field(rng, (3, 12, 300)), SLAT12, np.arange(300) * 1.2 + 0.4, tlat, tlon)
    assert len(set(tlat)) < len(tlat) and len(set(tlon)) < len(tlon) and c.nlon_t == 305 and c.W == 1
    assert [staged(s) for _, s, _ in c.spans] == [False, True]    # unsorted: a window nearly as wide as the 300-column source
    return c


def case_regional_nodes():
    """A 10 x 20 subgrid, not periodic; targets on every node (the first: dx == 0, the others: dx == Dx), a NaN cell
    whose neighbours' targets see it with weight 0."""
    rng = np.random.default_rng(61)
    slat, slon = 40.0 + np.arange(10), 5.0 + np.arange(20)
    f = _field(rng, (2, 10, 20))
    f[0, 4, 7] = np.nan
    f[1, 1, 1] = np.nan                                             # next to the first node of both axes
    beside = 1e-9
    tlat = np.concatenate([slat, [43.5, 45.0 - beside, 45.0 + beside, 43.0 + beside]])
    tlon = np.concatenate([slon, [11.5, 13.0 - beside, 13.0 + beside, 11.0 + beside, 24.0 - beside]])
    c = Case(f, slat, slon, tlat, tlon)
    tb = c.tb
    assert not tb['periodic'] and tb['south_row'] == tb['north_row'] == -1
    for ax, n in (('lat', 10), ('lon', 20)):
        dx, Dx = tb[ax + '_dx'][:n], tb[ax + '_Dx'][:n]
        assert dx[0] == 0.0 and (dx[1:] == Dx[1:]).all() and (Dx == 1.0).all() and not tb[ax + '_oob'].any()
    ref, _ = c.reference()
    nan = np.isnan(ref)
    # weight 0, NaN all the same: the node above / right of the NaN cell (dx == Dx, the cell is the LOWER neighbour)
    assert nan[0, 5, 7] and nan[0, 4, 8] and nan[0, 4, 7]
    assert not nan[0, 3, 7] and not nan[0, 4, 6]                   # the node below / left: its lower neighbour is another cell
    assert nan[1, 0, 1] and nan[1, 1, 0] and nan[1, 0, 0]          # the first node (dx == 0) has the cell as UPPER neighbour
    # just beside a node: 45 - d has the NaN row as LOWER neighbour, 45 + d does not; likewise 13 -+ d in longitude
    assert nan[0, 11, 7] and not nan[0, 12, 7] and nan[0, 4, 21] and not nan[0, 4, 22]
    assert 0 < nan.sum() < nan.size // 4
    return c


def case_both_extensions():
    """Source longitudes 20 .. 379, targets -30 .. 390: the copy at +360 and the copy at -360 are both used."""
    rng = np.random.default_rng(71)
    slon = 20.0 + np.arange(360)
    tlon = np.concatenate([np.arange(-30.0, 390.01, 0.7), [-30.0, 19.0, 20.0, 379.0, 380.0, 390.0]])
    c = Case(_field(rng, (2, 12, 360)), SLAT12, slon, np.array([-60.0, 0.5, 60.0]), tlon)
    assert c.tb['periodic'] and tlon.min() < slon.min() and tlon.max() > slon.max()
    below, above = tlon < slon.min(), tlon > slon.max()
    assert below.sum() > 50 and above.sum() > 10
    assert (c.tb['lon_lo'][below] >= 309).all() and (c.tb['lon_hi'][above] <= 11).all()       # folded back into the source
    assert not c.tb['lon_oob'].any()
    return c


CASES = {
    'window 765': case_window_765, 'window 768': case_window_768, 'window 765 vec1': case_window_765_vec1,
    'window 765 odd': case_window_765_odd,
    'gap W2': case_seam_gap_w2, 'gap W1': case_seam_gap_w1, 'seam mid block': case_seam_mid_block,
    'seam staged W2': case_seam_staged_w2,
    'pole south only': case_pole_south_only, 'pole north only': case_pole_north_only, 'pole none': case_pole_none,
    'pole in source': case_pole_in_source,
    'descending source': case_descending_source, 'descending targets': case_descending_targets,
    'descending both': case_descending_both, 'unsorted duplicate targets': case_unsorted_duplicate_targets,
    'regional nodes': case_regional_nodes, 'both extensions': case_both_extensions,
}
SLICE_NFIELDS = [1, 7, 8, 9, 16, 19, 40]
for _n in SLICE_NFIELDS:
    CASES['slices %d' % _n] = functools.partial(case_slices, _n)
POLE_CASES = ['pole south only', 'pole north only', 'pole none', 'pole in source']


@functools.lru_cache(maxsize=None)
def get_case(name):
    """The case, built (and its condition asserted) once per process; its references are cached on it."""
    return CASES[name]()


def oob_tables(c, lat_rows, lon_cols):
    """Case 8: the case's tables with `lat_oob` / `lon_oob` set at the given rows / columns; the indices stay as they are,
    inside the source grid."""
    tb = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in c.tb.items()}
    tb['lat_oob'][list(lat_rows)] = 1
    tb['lon_oob'][list(lon_cols)] = 1
    return tb


def case_oob(force_vec1):
    """(case, tables): a whole block of out-of-bounds targets, a block whose first valid target is not its first thread's
    first, flagged columns inside a staged and inside a direct block, two flagged rows."""
    c = get_case('window 765 vec1' if force_vec1 else 'window 765')
    per_block = BLOCK * c.W
    cols = list(range(0, 5)) + list(range(512, 1024)) + [1100, 1101, 1535]
    tb = oob_tables(c, [1, 4], cols)
    spans = block_spans(tb, c.nlon_s, c.nlon_t, c.W)
    assert any(s == (0, 0, per_block) for s in spans)                         # no valid target: s_first stays BLOCK * W
    assert spans[0][2] == 5 and spans[0][2] // c.W > 0 and spans[0][2] % c.W == c.W - 1      # W = 2: the second value of thread 2
    assert spans[0][0] == c.tb['lon_lo'][5] and 0 < spans[0][1] <= REGRID_SPAN
    assert any(0 < s[1] for s in spans[1:])
    if c.W == 2:
        assert not staged(spans[2][1])                                        # flagged columns in a direct block too
    assert (tb['lon_lo'] >= 0).all() and (tb['lon_hi'] < c.nlon_s).all()
    return c, tb


# ------------------------------------------------------------------ host tests
def oracle(c):
    with np.errstate(divide='ignore', invalid='ignore'):          # x_hi - x_lo == 0 of the pole-in-source case
        return O.regrid_lat_lon(c.field, c.src_lat, c.src_lon, c.targ_lat, c.targ_lon)


def _against_oracle(c):
    ref, bound = c.reference()
    want = oracle(c)
    assert want.shape == ref.shape
    nan = np.isnan(ref)
    np.testing.assert_array_equal(np.isnan(want), nan, err_msg='NaN mask')
    err = np.abs(want[~nan].astype(LD) - ref[~nan])
    assert (err <= bound[~nan]).all(), 'worst %.3f of the bound' % float((err / bound[~nan]).max())
    record('oracle vs reference', err, bound[~nan])
    return ref, bound, want


@pytest.fixture(scope='module', autouse=True)
def _report():
    yield
    if WORST:
        print('\nlargest observed error as a fraction of the derived bound: ' + ', '.join('%s %.3f' % kv for kv in sorted(WORST.items())))


@pytest.mark.parametrize('name', sorted(CASES))
def test_case_condition_and_reference_against_oracle(name):
    """The builder asserts the case's own condition; the longdouble reference agrees with the oracle within the bound
    derived from the oracle's float64 arithmetic, NaN masks equal."""
    c = get_case(name)
    ref, bound, want = _against_oracle(c)
    assert ref.shape == c.field.shape[:-2] + (c.nlat_t, c.nlon_t)
    finite = ~np.isnan(ref)
    assert finite.any() and (bound[finite] < 1e-11 * (1 + np.abs(ref[finite]))).all()       # the bound is a rounding bound


@pytest.mark.parametrize('name', sorted(CASES))
def test_kernel_statement_against_reference(name):
    """The float64 restatement of the kernel on the host tables is within the same bound of the reference (numpy's own
    zonal means as pole values) - and equal to the oracle's bits away from the pole rows, as the issue states."""
    c = get_case(name)
    ref, bound = c.reference()
    got = kernel_statement(c.field, c.tb, c.numpy_poles()).reshape(ref.shape)
    nan = np.isnan(ref)
    np.testing.assert_array_equal(np.isnan(got), nan, err_msg='NaN mask')
    err = np.abs(got[~nan].astype(LD) - ref[~nan])
    assert (err <= bound[~nan]).all(), 'worst %.3f of the bound' % float((err / bound[~nan]).max())
    record('kernel statement vs reference', err, bound[~nan])
    want = oracle(c)
    np.testing.assert_array_equal(got[..., ~c.pole_rows, :], want[..., ~c.pole_rows, :])


@pytest.mark.parametrize('name', ['window 765', 'pole south only', 'regional nodes'])
def test_float32_reference(name):
    """float32 storage: the reference of the widened inputs; its bound is the float64 one plus one float32 rounding."""
    c = get_case(name)
    ref, bound = c.reference(np.float32)
    ref64, bound64 = regrid_reference(c.typed(np.float32).astype(np.float64), c.src_lat, c.src_lon, c.targ_lat, c.targ_lon)
    np.testing.assert_array_equal(ref, ref64)
    nan = np.isnan(ref)
    assert (bound[~nan] >= bound64[~nan] + LD(2.0 ** -24) * np.abs(ref[~nan]) * (1 - 1e-15)).all()
    got = kernel_statement(c.typed(np.float32), c.tb, c.numpy_poles(np.float32)).reshape(ref.shape)
    assert got.dtype == np.float32
    np.testing.assert_array_equal(np.isnan(got), nan)
    assert (np.abs(got[~nan].astype(LD) - ref[~nan]) <= bound[~nan]).all()


def test_block_spans_and_slices_helpers():
    """The helpers on inputs whose answer is known by hand."""
    tb = dict(lon_lo=np.array([3, 4, 4, 0], dtype=np.int32), lon_hi=np.array([4, 0, 0, 1], dtype=np.int32),
              lon_oob=np.array([1, 0, 0, 0], dtype=np.int32))
    assert block_spans(tb, 5, 4, 1) == [(4, 3, 1)]                # c0 = 4; offsets 0, 1 (col 0), 2 (col 1)
    tb['lon_oob'][:] = 1
    assert block_spans(tb, 5, 4, 2) == [(0, 0, 512)]
    assert slices(228, 721, 1440, 2) == dict(bx=3, gz=8, per=29, sizes=[29] * 7 + [25])       # the full-size test's launch
    assert slices(1, 5, 8, 2)['gz'] == 1 and slices(3, 5, 1536, 2) == dict(bx=3, gz=3, per=1, sizes=[1, 1, 1])
    assert launch_w(1536) == 2 and launch_w(1535) == 1 and launch_w(1536, True) == 1


def test_oob_case_conditions():
    for force_vec1 in (False, True):
        c, tb = case_oob(force_vec1)
        got = kernel_statement(c.field, tb, c.numpy_poles())
        clean = kernel_statement(c.field, c.tb, c.numpy_poles())
        flagged = np.zeros(got.shape, dtype=bool)
        flagged[:, tb['lat_oob'] != 0, :] = True
        flagged[:, :, tb['lon_oob'] != 0] = True
        assert np.isnan(got[flagged]).all() and 0 < flagged.sum() < flagged.size
        np.testing.assert_array_equal(got[~flagged], clean[~flagged])
        assert not np.isnan(clean[~flagged]).any()


def test_reference_raises_like_the_tables():
    c = get_case('pole none')
    for kw in (dict(targ_lat=np.array([-89.0, 0.0]), src_lat=SLAT12[::-1]), dict(targ_lon=np.array([10.0, 150.0]), src_lon=SLON70[:20])):
        a = dict(src_lat=c.src_lat, src_lon=c.src_lon, targ_lat=c.targ_lat, targ_lon=c.targ_lon)
        a.update(kw)
        f = c.field[..., ::1, :len(a['src_lon'])]
        for fn in (lambda: regrid_reference(f, **a), lambda: regrid_tables(**a), lambda: O.regrid_lat_lon(f, **a)):
            with pytest.raises(ValueError):
                fn()
