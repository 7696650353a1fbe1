"""Data and the statement of correctness for the tests of postproc_cosmo.extpar_adapt (`pgw_time_mean_add`).

The statement is the literal numpy expression of the reference's postproc_cosmo/extpar_adapt.py:29-32 in its environment
(xarray 2022.12 without bottleneck: `.mean(dim=['time'])` of a float array is `np.nanmean(values, axis=0)`; netCDF4 hands
T_CL over as a masked array whose mask is `data == _FillValue / missing_value`, and `+=` is numpy's in-place add on it).
numpy is importable here and pins the arithmetic; netCDF4's masking rule is restated, not executed.  `python_loop` is the
per-cell rule written above k_time_mean_add, so that the kernel's documented rule is tied to numpy on the CPU.

Everything is compared bit for bit on unsigned views.  One thing is left open on purpose: WHICH NaN a 0 / 0 or a NaN + x
produces (sign and payload differ between processors, IEEE 754 leaves them free), so in cells the rule computes, NaN
compares equal to NaN; cells the rule leaves alone (masked) are compared as raw bits, NaN payloads included."""
import functools
import warnings

import numpy as np

F32, F64 = np.dtype('float32'), np.dtype('float64')
PAIRS = [(F32, F32), (F32, F64), (F64, F32), (F64, F64)]              # (dtype of base, dtype of the records)
N_CELLS = [1, 63, 64, 65, 257, 1030, 1032]                             # the tail of a wave, of a block, of the 16-byte form
N_REC = [1, 2, 8, 9, 12, 13]                                           # around CLIM_UNROLL = 8
NAN_PATTERNS = ['none', 'one_record_of_a_cell', 'all_records_of_a_cell', 'first_record_only', 'a_whole_record', 'negative_zeros']
MASKS = ['none', 'one_value', 'two_values', 'nan_value', 'every_cell']
NC_FILL = 9.969209968386869e36


def uview(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def same_bits(got, want, raw=None):
    """dtype, shape and bits equal; NaN equals NaN except where `raw` (bool array) asks for the raw words."""
    got, want = np.asarray(got), np.asarray(want)
    if got.dtype != want.dtype or got.shape != want.shape:
        return False
    g, w = uview(got).copy(), uview(want).copy()
    free = np.isnan(got) & np.isnan(want)
    if raw is not None:
        free &= ~np.asarray(raw).reshape(got.shape)
    g[free] = w[free] = 0
    return np.array_equal(g, w)


# ---- the statement ---------------------------------------------------------------------------------------------------------
def nanmean(x):
    with np.errstate(all='ignore'), warnings.catch_warnings():
        warnings.simplefilter('ignore')
        return np.nanmean(x, axis=0)


def mask_of(base, mask_values):
    """netCDF4's automatic mask: cells equal to a mask value after its conversion to the variable's dtype; a NaN value masks
    the NaN cells."""
    m = np.zeros(base.shape, dtype=bool)
    for v in mask_values:
        with np.errstate(all='ignore'):
            v = base.dtype.type(v)
        m |= np.isnan(base) if np.isnan(v) else (base == v)
    return m


def statement(base, x, mask_values=()):
    """-> (out, mean, n_masked, n_new_nan): the numpy expression, the counts counted on its result."""
    mean = nanmean(x)
    mask = mask_of(base, mask_values)
    ma = np.ma.masked_array(base.copy(), mask)
    with np.errstate(all='ignore'):
        ma += mean.squeeze()
    out = np.asarray(ma.data)
    out[mask] = base[mask]                                   # a masked cell is not touched (numpy adds 0 there)
    new_nan = ~mask & ~np.isnan(base) & np.isnan(out)
    return out, mean, int(mask.sum()), int(new_nan.sum())


def numpy_pairwise(a, T):
    """numpy's pairwise_sum on the list `a` of scalars of type T, as written above np_pairwise_sum in pgw_kernels.h."""
    n = len(a)
    if n < 8:
        res = T(0.0)
        for v in a:
            res = T(res + v)
        return res
    if n <= 128:
        r = list(a[:8])
        i = 8
        while i < n - n % 8:
            for j in range(8):
                r[j] = T(r[j] + a[i + j])
            i += 8
        res = T(T(T(r[0] + r[1]) + T(r[2] + r[3])) + T(T(r[4] + r[5]) + T(r[6] + r[7])))
        for v in a[i:]:
            res = T(res + v)
        return res
    n2 = n // 2
    n2 -= n2 % 8
    return T(numpy_pairwise(a[:n2], T) + numpy_pairwise(a[n2:], T))


def python_loop(base, x, mask_values=()):
    """Steps 1-4 of the per-cell rule, one IEEE operation per line, in numpy scalars of the stated types; a grid of one
    cell is summed in numpy's pairwise order (k_time_mean_add_one)."""
    X, B = x.dtype.type, base.dtype.type
    P = np.result_type(x.dtype, base.dtype).type
    flat_b, flat_x = base.reshape(-1), x.reshape(x.shape[0], -1)
    out, mean = np.empty(flat_b.shape, base.dtype), np.empty(flat_b.shape, x.dtype)
    with np.errstate(all='ignore'):
        mv = [B(v) for v in mask_values]
        for i in range(flat_b.size):
            xs = [X(0.0) if np.isnan(v) else v for v in flat_x[:, i]]
            tot, cnt = X(0.0), sum(0 if np.isnan(v) else 1 for v in flat_x[:, i])
            if flat_b.size == 1:
                tot = X(tot + numpy_pairwise(xs, X))
            else:
                for v in xs:
                    tot = X(tot + v)
            mean[i] = X(np.float64(tot) / np.float64(cnt))
            b = flat_b[i]
            if any((np.isnan(b) if np.isnan(m) else b == m) for m in mv):
                out[i] = b
            else:
                out[i] = B(P(b) + P(mean[i]))
    return out.reshape(base.shape), mean.reshape(x.shape[1:])


# ---- the data --------------------------------------------------------------------------------------------------------------
def _uniform(nrec, n, dtype, seed):
    return np.random.default_rng(seed).uniform(0.5, 6.0, (nrec, n)).astype(dtype)


def flow_shares(ncell=4000, seed=0):
    """Share of cells in which (a) the float32 record-order sum differs from the float64 sum rounded once, (b) the float32
    sum in record order differs from the one in reversed order, (c) the same for float64 data - on 12 records of the data
    `records` hands out."""
    x32, x64 = _uniform(12, ncell, F32, seed), _uniform(12, ncell, F64, seed)

    def ordered(x, order):
        tot = x[order[0]].copy()
        for r in order[1:]:
            tot = tot + x[r]
        return tot
    fwd, rev = list(range(12)), list(range(11, -1, -1))
    a = (ordered(x32, fwd) != ordered(x32.astype(F64), fwd).astype(F32)).mean()
    b = (ordered(x32, fwd) != ordered(x32, rev)).mean()
    c = (ordered(x64, fwd) != ordered(x64, rev)).mean()
    return float(a), float(b), float(c)


@functools.lru_cache(maxsize=None)
def check_data_tells_flows_apart():
    """The condition under which a bit-for-bit comparison can tell the dtype flows and the summation orders apart: each
    share at least a quarter (measured 0.54, 0.51, 0.51)."""
    shares = flow_shares()
    assert min(shares) >= 0.25, shares
    return shares


def records(nrec, n, dtype, pattern='none', seed=0):
    """x (nrec, n) of uniform(0.5, 6.0) values with the NaN pattern."""
    check_data_tells_flows_apart()
    x = _uniform(nrec, n, dtype, seed + 1000 * nrec + n)
    rng = np.random.default_rng(seed + 7)
    some = rng.random(n) < 0.4
    some[n // 2] = True
    if pattern == 'one_record_of_a_cell':
        x[rng.integers(0, nrec, n)[some], np.nonzero(some)[0]] = np.nan
    elif pattern == 'all_records_of_a_cell':
        x[:, some] = np.nan
    elif pattern == 'first_record_only':
        x[0, some] = np.nan
    elif pattern == 'a_whole_record':
        x[nrec // 2] = np.nan
    elif pattern == 'negative_zeros':
        x[:, some] = -0.0
        x[rng.integers(0, nrec, n)[some], np.nonzero(some)[0]] = np.nan
        x[:, 0] = -0.0                                       # and one cell of -0.0 alone: numpy's sum starts from +0.0
    elif pattern != 'none':
        raise ValueError(pattern)
    return x


def base_and_mask(n, dtype, kind, seed=0):
    """-> (base (n), mask values): temperatures around 280 K, some cells holding a mask value."""
    rng = np.random.default_rng(seed + 31 * n)
    base = rng.uniform(265.0, 295.0, n).astype(dtype)
    hit = rng.random(n) < 0.3
    hit[n - 1] = True
    if kind == 'none':
        return base, []
    if kind == 'one_value':
        base[hit] = -1.0e20
        return base, [-1.0e20]
    if kind == 'two_values':
        base[hit] = np.where(rng.random(int(hit.sum())) < 0.5, -1.0e20, NC_FILL).astype(dtype)
        return base, [-1.0e20, NC_FILL]
    if kind == 'nan_value':
        base[hit] = np.nan
        return base, [np.nan]
    if kind == 'every_cell':
        base[:] = -999.0
        return base, [-999.0]
    raise ValueError(kind)
