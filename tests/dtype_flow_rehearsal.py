"""The reference's surface-pressure loop (step_03_apply_to_era.py:182-319) written out with FUNCTION CALLS, as an import
swap of the reference's own script would run it: numpy arithmetic exactly as the reference has it (`delta_ps` / `adj_ps` as
`zeros_like(PS)`, the in-place `+=`, `ps_pgw = PS + delta_ps`), the two functions that carry the work -
`relative_to_specific_humidity` and `integ_geopot` - handed in.  Shared by tests/test_function_dtype_flow_host.py (which
pins this loop against the reference-dtype oracle's own) and tests/test_function_dtype_flow.py (which runs it on the GPU
functions).  Not a test module."""
import numpy as np

from oracle import pgw_oracle as O
from oracle import pgw_oracle_refdtype as R

SHAPES = [((10, 10, 20), 0), ((24, 36, 60), 1), ((7, 13, 21), 2), ((3, 5, 137), 3)]


def f32_case(shape, seed):
    from pgw4era5_amd import synthetic
    nlat, nlon, nlev = shape
    return synthetic.make_case(nlat=nlat, nlon=nlon, nlev=nlev, seed=seed, dtype=np.float32)


def oracle_file_run(case):
    """The reference-dtype oracle's whole-file run and the loop's inputs taken from it: (run, ta_pgw, hur_pgw, dzg)."""
    run = R.pgw_for_era5_arrays(case['era'], case['deltas'], case['delta_times'], case['plev'], case['target_dt'], True)
    times = case['delta_times']
    zg = R.load_delta_values(case['deltas']['zg'], times['zg'] if isinstance(times, dict) else times, case['target_dt'])
    plev = np.asarray(case['plev'], dtype=np.float64)
    k = int(np.nonzero(plev == O.P_REF_INP)[0][0])
    return run, run['T'], run['RELHUM_pgw'], zg[:, k]


def rehearsal(relative_to_specific_humidity, integ_geopot, era, ta_pgw, hur_pgw, dzg_pref):
    """step_03:182-319 with fixed p_ref; returns dict(n_iter, max_err, PS)."""
    ak, bk = np.asarray(era['ak']), np.asarray(era['bk'])
    akm, bkm = era.get('akm'), era.get('bkm')
    if akm is None:
        akm, bkm = R.full_level_coeffs(ak, bk)
    PS, FIS, T, QV = era['PS'], era['FIS'], era['T'], era['QV']
    p_ref = O.P_REF_INP
    level1 = np.arange(1, len(ak) + 1)
    pa_hl_era, _ = R.hybrid_pressure(ak, bk, PS, akm, bkm)                          # :64-66
    delta_ps = np.zeros_like(PS)                                                    # :182
    adj_ps = np.zeros_like(PS)                                                      # :184
    phi_ref_max_error = np.inf
    it = 1
    hist = []
    while phi_ref_max_error > O.THRESH_PHI_REF_MAX_ERROR:
        delta_ps += adj_ps                                                          # :192
        ps_pgw = PS + delta_ps                                                      # :193
        pa_hl_pgw, pa_pgw = R.hybrid_pressure(ak, bk, ps_pgw, akm, bkm)             # :196-199
        hus_pgw = relative_to_specific_humidity(hur_pgw, pa_pgw, ta_pgw)            # :262-266
        phi_ref_pgw = integ_geopot(pa_hl_pgw, FIS, ta_pgw, hus_pgw, level1, p_ref)  # :269-276
        phi_ref_era = integ_geopot(pa_hl_era, FIS, T, QV, level1, p_ref)            # :280-287
        delta_phi_ref = phi_ref_pgw - phi_ref_era                                   # :289
        climate_delta_phi_ref = dzg_pref * O.CON_G                                  # :292-295
        phi_ref_error = delta_phi_ref - climate_delta_phi_ref                       # :298
        adj_ps = - O.ADJ_FACTOR * ps_pgw / (O.CON_RD * ta_pgw[:, -1]) * phi_ref_error   # :301-304
        phi_ref_max_error = np.nanmax(np.abs(phi_ref_error))                        # :308
        hist.append(float(phi_ref_max_error))
        it += 1
        if it > O.MAX_N_ITER:                                                       # :313-319
            raise ValueError('ERROR! Pressure adjustment did not converge')
    return dict(n_iter=it - 1, max_err=hist, PS=ps_pgw)
