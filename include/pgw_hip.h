/*
 * pgw_hip.h  --  C-ABI of libpgw_hip.so: the MI355X (gfx950) compute path for the
 * PGW4ERA5 step_03 / step_02 hot path.
 *
 * Every entry point replaces one piece of the reference's Python interface; the
 * citation after each declaration is the reference file:line it stands in for
 * (paths relative to the reference repository root).  The reference has no FFI of
 * its own (it is pure Python); the binding a maintainer adds is the ctypes stub shown
 * in INTEGRATION.md (pgw4era5_amd/_lib.py is that stub in full).
 *
 * Conventions
 *  - plain C: opaque context, raw pointers, sizes; no C++/torch types.
 *  - all `field` pointers are DEVICE pointers (from pgw_malloc or any hipMalloc'd
 *    buffer, e.g. a torch tensor's data_ptr()); small coefficient vectors (ak, bk,
 *    plev, coordinate tables) are HOST pointers, copied by the call.
 *  - `dtype` is the STORAGE type of field arrays (PGW_F32 / PGW_F64); arithmetic is
 *    always IEEE fp64, no fast-math.
 *  - 4-D fields are C-order (time, level, lat, lon); `ncol` = nlat*nlon; pressure
 *    ascends with the level index (functions.py:500-503 of the reference).
 *  - calls on one context are stream-ordered on the context's HIP stream and are not
 *    re-entrant; functions that report data errors synchronise before returning.
 *  - return value: 0 = PGW_OK, otherwise a pgw_status code; pgw_last_error() gives
 *    the text, pgw_error_column() the first offending column (or -1).
 */
#ifndef PGW_HIP_H
#define PGW_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct pgw_ctx pgw_ctx;

enum pgw_status {
    PGW_OK = 0,
    PGW_ERR_HIP = 1,                 /* HIP runtime failure (text in pgw_last_error)            */
    PGW_ERR_ARG = 2,                 /* bad argument / shape (functions.py:407-412,457-465)     */
    PGW_ERR_SRC_NOT_ASCENDING = 10,  /* 'Source pressure values must be ascending!'  :500-501   */
    PGW_ERR_TARG_NOT_ASCENDING = 11, /* 'Target pressure values must be ascending!'  :502-503   */
    PGW_ERR_EXTRAP_OFF = 12,         /* 'Extrapolation deactivated but data out of bounds.' :564 */
    PGW_ERR_PREF_BELOW_SURFACE = 13, /* 'p_ref locally lies below the surface...'    :162-165   */
    PGW_ERR_PREF_AT_TOP = 14,        /* k* = 0: tav.sel(level=0) KeyError            :176       */
    PGW_ERR_PS_HIST_ABOVE_TOP = 15,  /* replace_delta_sfc ValueError()               :360-363   */
    PGW_ERR_TOP_PRESSURE = 16,       /* 'ERA5 top pressure is lower than ...'        :417-425   */
    PGW_ERR_NOT_CONVERGED = 17,      /* 'Pressure adjustment did not converge' step_03:313-319  */
    PGW_ERR_GRID_EXTENT = 18,        /* regrid: target exceeds source    functions.py:845-888   */
    PGW_ERR_NO_P_REF = 19,           /* 'No reference pressure level above ...'  step_03:245-251 */
    PGW_ERR_REDUCE = 20              /* the caller's reduce hook (pgw_set_reduce_hook) returned non-zero               */
};

enum pgw_dtype { PGW_F32 = 0, PGW_F64 = 1 };

/* interp_logp_4d `extrapolate` argument (functions.py:434-446) */
enum pgw_extrap { PGW_EXTRAP_OFF = 0, PGW_EXTRAP_LINEAR = 1, PGW_EXTRAP_CONSTANT = 2, PGW_EXTRAP_NAN = 3 };

/* kernel ids for the per-context launch profiler (pgw_profile_*) */
enum pgw_kernel_id {
    PGW_K_PRESSURE = 0, PGW_K_Q_TO_RH = 1, PGW_K_RH_TO_Q = 2, PGW_K_INTEG_GEOPOT = 3,
    PGW_K_INTERP_LOGP = 4, PGW_K_TIME_LERP = 5, PGW_K_VERT_INTERP_DELTA = 6,
    PGW_K_ADJUST_PS_STEP = 7, PGW_K_REGRID = 8, PGW_K_SURFACE = 9, PGW_K_FINALIZE = 10,
    PGW_K_THERMO_DELTA = 11, PGW_K_WIND_DELTA = 12, PGW_K_PHI_REF_HYBRID = 13, PGW_K_QUAD_DELTA = 14,
    PGW_K_BYTESWAP = 15, PGW_K_HARMONIC = 16, PGW_K_GAUSS_INTERP = 17, PGW_K_PS_LOOP_MULTI = 18,
    PGW_K_HYBRID_TO_PLEV = 19, PGW_K_MAGNUS_RH = 20, PGW_K_HUR_MERGE = 21,
    PGW_K_CLIM_ACCUMULATE = 22, PGW_K_FIELD_SUB = 23, PGW_K_CLIM_READ = 24, PGW_K_DELTA_FIELDS = 25,
    PGW_K_CELL_LOCATE = 26, PGW_K_REGRID_SPARSE = 27,
    PGW_K_COUNT = 28
};

/* per-context options (pgw_set_option).  Defaults come from the environment variables named below, which are read
 * ONCE, in pgw_ctx_create; nothing on the launch path calls getenv. */
enum pgw_option {
    PGW_OPT_QUAD = 0,         /* 1 (default): ta+hur and ua+va deltas in one kernel; 0: the two pair kernels   [PGW_QUAD]        */
    PGW_OPT_FULL_COLUMN = 1,  /* 1: loop passes read every level (input-independent traffic); default 0: a wave stops once
                                 all its columns are above p_ref                                                 [PGW_FULL_COLUMN] */
    PGW_OPT_FORCE_VEC1 = 2,   /* 1: one column per thread everywhere (test knob for the scalar-column code path)  [PGW_FORCE_VEC1]  */
    PGW_OPT_MULTIPASS = 3,    /* 1 (default): several passes of the surface-pressure loop per launch with the column held
                                 on chip; 0: one launch per pass                                                 [PGW_MULTIPASS]   */
    PGW_OPT_LOOP_GUESS = 4,   /* passes the next file's first multi-pass launch runs (1..8); updated by every file to its own pass
                                 count (consecutive ERA5 files of a run need the same number); initial value 6                  */
    PGW_OPT_FORCE_OFF64 = 5,  /* 1: the 64-bit byte-offset instantiations of the kernels that address arrays below 4 GiB with
                                 32-bit offsets (k_delta_quad, k_reinterp_pair) - test knob: the path a 0.125 deg L137 file takes    */
    PGW_OPT_TEST_FAIL = 6,    /* test knob, default 0: pgw_step03_file fails on purpose - 1: the loop's workspace (ws_get), 2: before the
                                 first loop launch, 3: before a continuation launch - so that the latitude-band protocol can be
                                 tested where one band stops on its own                                                           */
    PGW_OPT_FUSED_FIRST = 7,  /* 1 (default): in pgw_step03_file the delta kernel, which walks every column from the surface up, also
                                 runs the loop's first two scans (phi_ref of the ERA state, pass 1) on the levels it holds in
                                 registers; 0: the first loop launch does.  Same bits either way (see pgw_step03_file).  Takes
                                 effect with PGW_OPT_QUAD = 1, PGW_OPT_MULTIPASS = 1, PGW_OPT_FULL_COLUMN = 0, a fixed p_ref
                                 and i_reinterp = 0                                                              [PGW_FUSED_FIRST] */
    PGW_OPT_MIXED_VEC = 8,    /* columns / elements per thread of the `_mixed` entries (operands of different element size), cap:
                                 4 (default): a float32 row is one 16-byte access per lane, a float64 row beside it two; 2: 8 and
                                 16 bytes; 1: scalar.  A/B knob of tools/function_flow_time.py                                       */
    PGW_OPT_SPARSE_DIRECT = 9, /* test knob, default 0: pgw_regrid_sparse stages a block's source window in LDS when it fits; 1: every
                                 block gathers from memory.  Same bits either way                                                     */
    PGW_OPT_QV_FROM_PASS = 10, /* 1 (default): the last pass of every multi-pass loop launch (fixed p_ref) also stores the QV it forms
                                 below p_ref into hus_pgw; when that pass is the converged one - the host predicts it with
                                 PGW_OPT_LOOP_GUESS - the finalize kernel computes only the levels above it (pgw_last_qv_from_pass),
                                 otherwise all of them as with 0.  Same bits either way for every divisor pm - 0.378 e that is a finite
                                 pressure of normal range and every e >= 0 that is 0 or of normal range; outside that - a divisor of
                                 exactly 0 or inf, denormal-scale operands, e = -0 - the pass's scale-free quotient can differ from
                                 the finalize kernel's IEEE division (NaN for inf, +0 for -0), as k_delta_quad's QV of the
                                 pure-pressure levels already does.  Takes effect with PGW_OPT_MULTIPASS = 1,
                                 PGW_OPT_FULL_COLUMN = 0, a fixed p_ref, i_reinterp = 0, in pgw_step03_file with PGW_OPT_QUAD = 1, and
                                 for float64 level arrays (float64 files, float32 files in reference-dtype mode)  [PGW_QV_FROM_PASS] */
    PGW_OPT_FINISH_IN_PASS = 11, /* 1 (default): the end of a file on the production path.  The storing pass of PGW_OPT_QV_FROM_PASS
                                 goes on from where its scan stopped to the first hybrid level and writes ps_pgw, so a file whose
                                 predicted pass converges launches no finalize kernel (pgw_last_qv_from_pass: 1, every hybrid
                                 level-column skipped); any other stop runs the finalize kernel over all levels as before (float64
                                 files only: float32 files in reference-dtype mode keep the finalize kernel with its marks).  And
                                 pgw_step03_file (PGW_OPT_QUAD = 1, fixed p_ref, i_reinterp = 0, multi-pass loop) enqueues the
                                 surface riders behind the first loop launch's status read-back, where the stream would wait for
                                 the host, instead of first.  0: riders first, finalize kernel with marks.  Same bits either way
                                 under PGW_OPT_QV_FROM_PASS's conditions                                  [PGW_FINISH_IN_PASS] */
    PGW_OPT_COUNT = 12
};

/* ---------------------------------------------------------------- context ------------ */
/* One context = one HIP device + one stream; replaces the implicit per-process state of a
 * reference worker (parallel.py:18-32: one process per file, no shared state). */
int pgw_device_count(int *n);
/* PCI address ("0000:c1:00.0", NUL-terminated; len >= 13) of HIP device `device`: the key under /sys/bus/pci/devices/ whose
 * `numa_node` a rank binds its host threads and pinned buffers to (pgw4era5_amd/parallel.py bind_rank_to_numa).  The
 * reference's workers are unplaced `multiprocessing.Pool` processes (parallel.py:18-32). */
int pgw_device_pci_bus_id(int device, char *buf, int len);
int pgw_ctx_create(int device, pgw_ctx **out);
int pgw_ctx_destroy(pgw_ctx *ctx);
int pgw_set_option(pgw_ctx *ctx, int option, int value);
int pgw_get_option(pgw_ctx *ctx, int option, int *value);
/* One ERA5 file split into latitude bands over several contexts / ranks: the columns of
 * a file are independent except for the loop's stopping test, the maximum of |phi error| over ALL columns
 * (step_03_apply_to_era.py:189, 308).  With a hook set, pgw_step03_file hands the per-pass figures of its band to
 * `fn(vals, n, user)`, which must replace every element by its MAXIMUM over the ranks holding the file's other bands
 * (an 8..200-byte all-reduce per loop launch: RCCL / gloo in the caller, see pgw4era5_amd/parallel.py) and return 0.
 * Every rank then takes the same stopping decision, and an error status of one band is returned by all.  n is the same
 * on all ranks at every call.  fn = NULL removes the hook.  Needs the multi-pass loop (PGW_OPT_MULTIPASS = 1,
 * PGW_OPT_FULL_COLUMN = 0; fixed or local p_ref). */
typedef int (*pgw_reduce_max_fn)(double *vals, int n, void *user);
int pgw_set_reduce_hook(pgw_ctx *ctx, pgw_reduce_max_fn fn, void *user);
/* A band that cannot even call pgw_step03_file for the file all bands are about to process (its host-side set-up raised:
 * a failed upload, an out-of-memory) calls this instead: one reduce of the length the others' first loop launch makes,
 * carrying `code`, so that their pgw_step03_file returns `code` instead of waiting for this band until the collective
 * backend's timeout.  (A failure INSIDE pgw_step03_file does this by itself, whenever it happens.) */
int pgw_band_abort(pgw_ctx *ctx, int code, int max_n_iter);
const char *pgw_last_error(pgw_ctx *ctx);
long long pgw_error_column(pgw_ctx *ctx);
const char *pgw_version(void);
int pgw_device_name(pgw_ctx *ctx, char *buf, size_t len);

/* ---------------------------------------------------------------- memory / stream ---- */
int pgw_malloc(pgw_ctx *ctx, size_t bytes, void **dptr);
int pgw_free(pgw_ctx *ctx, void *dptr);
int pgw_host_alloc(pgw_ctx *ctx, size_t bytes, void **hptr);      /* pinned host memory */
int pgw_host_free(pgw_ctx *ctx, void *hptr);
int pgw_memcpy_h2d(pgw_ctx *ctx, void *dst, const void *src, size_t bytes);   /* async */
int pgw_memcpy_d2h(pgw_ctx *ctx, void *dst, const void *src, size_t bytes);   /* async */
int pgw_memcpy_d2d(pgw_ctx *ctx, void *dst, const void *src, size_t bytes);   /* async */
int pgw_memset(pgw_ctx *ctx, void *dst, int value, size_t bytes);             /* async */
int pgw_sync(pgw_ctx *ctx);
int pgw_mem_info(pgw_ctx *ctx, size_t *free_bytes, size_t *total_bytes);

/* HIP-event launch profiler: when enabled every kernel launched by this library is
 * bracketed by two events on the context stream; pgw_profile_get synchronises and returns
 * launch count and summed device time of kernel `kid` since the last reset. */
int pgw_profile_enable(pgw_ctx *ctx, int on);
int pgw_profile_reset(pgw_ctx *ctx);
int pgw_profile_get(pgw_ctx *ctx, int kid, long long *launches, double *total_ms);
int pgw_timer_start(pgw_ctx *ctx);                 /* event on the context stream */
int pgw_timer_stop(pgw_ctx *ctx, double *ms);      /* records, synchronises, returns elapsed */

/* ---------------------------------------------------------------- vertical grid ------ */
/* Hybrid coefficients of the ERA5 file: ak, bk on half levels (nlev+1 values), akm/bkm on
 * full levels (nlev values) or NULL -> 0.5*diff + lower, as step_03_apply_to_era.py:68-85.
 * Host pointers; kept in the context until the next call. */
int pgw_set_levels(pgw_ctx *ctx, int nlev, const double *ak, const double *bk,
                   const double *akm, const double *bkm);
int pgw_get_full_level_coeffs(pgw_ctx *ctx, double *akm_out, double *bkm_out);

/* a1 "integ_pressure": pa_hl = ak + ps*bk ; pa = akm + ps*bkm
 * (step_03_apply_to_era.py:64-66, 87-88, 196-199).  Either output may be NULL.
 * ps (ntime, ncol) ; pa_hl (ntime, nlev+1, ncol) ; pa (ntime, nlev, ncol). */
int pgw_pressure_levels(pgw_ctx *ctx, int dtype, int ntime, long long ncol,
                        const void *ps, void *pa_hl, void *pa);

/* ---------------------------------------------------------------- humidity ----------- */
/* a2 specific_to_relative_humidity(hus, pa, ta)   functions.py:107-116 (with :58-64,:74-105)
 * a3 relative_to_specific_humidity(hur, pa, ta)   functions.py:118-125 (with :66-72)
 * flat elementwise over n elements. */
int pgw_specific_to_relative_humidity(pgw_ctx *ctx, int dtype, long long n,
                                      const void *hus, const void *pa, const void *ta, void *hur);
int pgw_relative_to_specific_humidity(pgw_ctx *ctx, int dtype, long long n,
                                      const void *hur, const void *pa, const void *ta, void *hus);
/* the leaf helpers of the same block, for callers that use them directly (flat, n elements; b is ignored by 2..4):
 *   which = 0  specific_humidity_to_vapor_pressure(hus = a, pa = b)             functions.py:58-64
 *           1  vapor_pressure_to_specific_humidity(vapp = a, pa = b)            :66-72
 *           2  saturation_vapor_pressure_water_or_ice(pa, ta = a, water=True)   :74-89
 *           3  ... water=False (over ice)
 *           4  saturation_vapor_pressure_water_and_ice(pa, ta = a)              :91-105 */
int pgw_humidity_leaf(pgw_ctx *ctx, int dtype, int which, long long n, const void *a, const void *b, void *out);
/* same, with pa = akm + ps*bkm rebuilt in registers instead of read (saves the 4-D pa array
 * step_03:87-94 / :196-197,262-266 materialise).  fields (ntime, nlev, ncol), ps (ntime, ncol) */
int pgw_specific_to_relative_humidity_hybrid(pgw_ctx *ctx, int dtype, int ntime, long long ncol,
                                             const void *hus, const void *ps, const void *ta, void *hur);
int pgw_relative_to_specific_humidity_hybrid(pgw_ctx *ctx, int dtype, int ntime, long long ncol,
                                             const void *hur, const void *ps, const void *ta, void *hus);

/* ---------------------------------------------------------------- integ_geopot ------- */
/* a4 integ_geopot(pa_hl, zgs, ta, hus, level1, p_ref)     functions.py:128-189
 * pa_hl (ntime, nlev+1, ncol); zgs (ntime, ncol); ta, hus (ntime, nlev, ncol);
 * p_ref: scalar `p_ref`, or per-column field `p_ref_field` (ntime, ncol) when non-NULL;
 * phi_ref (ntime, ncol) out.  nlev = number of full levels (level1 labels are 1..nlev+1).
 * full_column != 0 reads every level of every column (signature-faithful traffic,
 * (3*nlev+3)*ncol elements, exact for any pressure ordering); 0 is the caller's assertion
 * that pressure ascends strictly with the level index, and lets a wave stop once all of its
 * columns have passed p_ref (identical results under that assertion). */
int pgw_integ_geopot(pgw_ctx *ctx, int dtype, int ntime, int nlev, long long ncol,
                     const void *pa_hl, const void *zgs, const void *ta, const void *hus,
                     double p_ref, const void *p_ref_field, void *phi_ref, int full_column);

/* ---------------------------------------------------------------- interp_logp_4d ----- */
/* a6 interp_logp_4d(var, source_P, targ_P, extrapolate)   functions.py:434-477 and the
 * column kernels :479-580.  var, source_P (ntime, nsrc, ncol); targ_P, out (ntime, ntarg, ncol).
 * logp_in == 0: pressures in, logs taken inside (:470-471) = interp_logp_4d;
 * logp_in != 0: the arrays already hold ln p = interp_1d_for_timelatlon (:479-508) and, with
 * ntime = ncol = 1, interp_extrap_1d (:511-580). */
int pgw_interp_logp_4d(pgw_ctx *ctx, int dtype, int ntime, int nsrc, int ntarg, long long ncol,
                       const void *var, const void *source_P, const void *targ_P,
                       int extrapolate, int logp_in, void *out);

/* ---------------------------------------------------------------- deltas ------------- */
#define PGW_MAX_PLEV 128       /* levels of the plev axis of ta / hur / ua / va deltas */
#define PGW_MAX_PLEV_ZG 64     /* levels of zg's plev axis (pgw_file_args.nplev_zg, pgw_geopot_on_plev) */
/* a7 the arithmetic of load_delta's time interpolation (functions.py:288-292 -> scipy
 * interp1d linear): out = (v_after - v_before)/x_hi * x_new + v_before, flat over n. */
int pgw_time_lerp(pgw_ctx *ctx, int dtype, long long n, const void *v_before, const void *v_after,
                  double x_hi, double x_new, void *out);

/* a8 vert_interp_delta(delta, target_P, delta_sfc, ps_hist, ignore_top)  functions.py:369-431
 * (+ replace_delta_sfc :343-366, + the time lerp of load_delta, + `era + delta` of
 * step_03_apply_to_era.py:170-173) fused per column.
 *  plev (nplev, host): the delta file's plev coordinate in FILE order; it is reversed like :383-384.
 *    2 <= nplev <= 128 (PGW_MAX_PLEV), here and in every entry below that takes the plev axis of a delta (the reference's
 *    step_01 writes 99 levels).  An axis of up to 64 levels runs the kernels built for a 64-entry table, a longer one their
 *    128-entry instantiations: same arithmetic, the table is a by-value kernel argument either way.
 *  delta_b / delta_a (nplev, ncol) per time: the two bracketing records (delta_a NULL, or
 *    x_hi == 0 -> delta_b is used as is, functions.py:282-283); same for the optional
 *    surface pairs dsfc_*, pshist_* (ntime, ncol) (NULL -> no surface insertion).
 *  target pressure: targ_P (ntime, nlev_t, ncol) if non-NULL, else akm + ps*bkm from
 *    pgw_set_levels with ps (ntime, ncol).
 *  add_to (ntime, nlev_t, ncol) or NULL: out = add_to + delta_interp.
 *  ignore_top != 0 skips the model-top check (:417-425). */
int pgw_vert_interp_delta(pgw_ctx *ctx, int dtype, int ntime, int nplev, int nlev_t, long long ncol,
                          const double *plev,
                          const void *delta_b, const void *delta_a, double x_hi, double x_new,
                          const void *dsfc_b, const void *dsfc_a,
                          const void *pshist_b, const void *pshist_a,
                          const void *targ_P, const void *ps,
                          int ignore_top, const void *add_to, void *out);

/* f3  settings.i_reinterp = 1, one variable of one loop pass (step_03_apply_to_era.py:202-216; ua / va after the loop,
 * :330-343):  out = interp_logp_4d(era_field, pa_era, pa_pgw, extrapolate='constant') + load_delta_interp(var, pa_pgw)
 * as ONE kernel: pa_era = akm + ps_era*bkm (source axis of the first term) and pa_pgw = akm + ps_pgw*bkm (target of
 * both) are rebuilt in registers from the two surface-pressure fields (ntime, ncol) and pgw_set_levels, the delta
 * arguments are those of pgw_vert_interp_delta (nplev up to 128).  era_field, out: (ntime, nlev, ncol). */
int pgw_reinterp_field(pgw_ctx *ctx, int dtype, int ntime, int nplev, long long ncol, const double *plev,
                       const void *delta_b, const void *delta_a, double x_hi, double x_new, const void *dsfc_b,
                       const void *dsfc_a, const void *pshist_b, const void *pshist_a, const void *era_field,
                       const void *ps_era, const void *ps_pgw, int ignore_top, void *out);

/* f3  the same for TWO variables that share both pressure axes - ta + hur (one ps_hist; step_03_apply_to_era.py:202-216)
 * or ua + va (:330-343; dsfc_b = NULL) - in one kernel: one target logarithm per level, one source logarithm per level of
 * the ERA column and one bracket search per axis serve both.  delta_b / delta_a / dsfc_b / dsfc_a / era_field / out are
 * arrays of two device pointers (dsfc_b, dsfc_a, delta_a may be NULL as in pgw_reinterp_field); results are the bits of
 * two pgw_reinterp_field calls.  nplev up to 128. */
int pgw_reinterp_pair(pgw_ctx *ctx, int dtype, int ntime, int nplev, long long ncol, const double *plev,
                      const void *const *delta_b, const void *const *delta_a, double x_hi, double x_new,
                      const void *const *dsfc_b, const void *const *dsfc_a, const void *pshist_b, const void *pshist_a,
                      const void *const *era_field, const void *ps_era, const void *ps_pgw, int ignore_top, void *const *out);

/* f3  one pass of the surface-pressure loop with settings.i_reinterp = 1 (step_03_apply_to_era.py:192-216, 262-308) in one
 * call and one host synchronisation: delta_ps += adj_ps, ps_pgw = PS + delta_ps (:192-193); ta_pgw / hur_pgw =
 * interp_logp_4d(T / RELHUM of the ERA state, pa_era, pa_pgw, 'constant') + load_delta_interp(ta / hur, pa_pgw) (:202-216,
 * pgw_reinterp_pair, which also leaves e = hur_pgw / 100 * e_sat(ta_pgw) in a workspace); then the pass of pgw_adjust_ps_step
 * on them: adj_ps and the global max |phi error| (:262-308).  Same bits as pgw_update_ps + pgw_reinterp_pair +
 * pgw_adjust_ps_step(apply_adj = 0).  ps_pgw (ntime, ncol), ta_pgw, hur_pgw (ntime, nlev, ncol) are outputs.  nplev up to 128. */
int pgw_reinterp_pass(pgw_ctx *ctx, int dtype, int ntime, int nplev, long long ncol, const double *plev,
                      const void *const *delta_b, const void *const *delta_a, double x_hi, double x_new,
                      const void *const *dsfc_b, const void *const *dsfc_a, const void *pshist_b, const void *pshist_a,
                      const void *T_era, const void *RELHUM_era, const void *PS, const void *FIS, const double *phi_ref_era,
                      const double *dphi_clim, double *delta_ps, double *adj_ps, double p_ref, double adj_factor,
                      int ignore_top, void *ps_pgw, void *ta_pgw, void *hur_pgw, double *max_abs_err);

/* replace_delta_sfc(source_P, ps_hist, delta, delta_sfc)  functions.py:343-366, on many columns:
 * plev_asc (nplev, host, ascending; 1 <= nplev <= 128); delta (ntime, nplev, ncol) in ascending order;
 * delta_sfc, ps_hist (ntime, ncol); outputs out_P, out_delta (ntime, nplev, ncol). */
int pgw_replace_delta_sfc(pgw_ctx *ctx, int dtype, int ntime, int nplev, long long ncol,
                          const double *plev_asc, const void *delta, const void *delta_sfc,
                          const void *ps_hist, void *out_P, void *out_delta);

/* ---------------------------------------------------------------- ps fixed-point loop - */
/* a5 one pass of the loop body step_03_apply_to_era.py:192-308 for fixed p_ref, fused:
 * delta_ps += adj_ps ; ps = PS + delta_ps ; pa, pa_hl ; hus = rh_to_q(hur_pgw, pa, ta_pgw) ;
 * phi_ref_pgw = integ_geopot(...) ; err = (phi_ref_pgw - phi_ref_era) - dphi_clim ;
 * adj_ps = -adj_factor*ps/(Rd*ta_pgw[lowest])*err ; max|err| (NaN skipped).
 *  ta_pgw, hur_pgw (ntime, nlev, ncol) storage dtype; PS, FIS (ntime, ncol) storage dtype;
 *  phi_ref_era, dphi_clim, delta_ps, adj_ps (ntime, ncol) DOUBLE (loop state is fp64);
 *  p_ref_field (double, (ntime,ncol)) or NULL -> scalar p_ref.
 *  max_abs_err (host out). */
int pgw_adjust_ps_step(pgw_ctx *ctx, int dtype, int ntime, long long ncol,
                       const void *ta_pgw, const void *hur_pgw, const void *PS, const void *FIS,
                       const double *phi_ref_era, const double *dphi_clim,
                       double *delta_ps, double *adj_ps,
                       double p_ref, const double *p_ref_field, double adj_factor,
                       int apply_adj, double *max_abs_err);
/* apply_adj != 0: the pass itself does delta_ps += adj_ps (step_03:192); 0: the caller already did
 * (pgw_update_ps), as needed when the model-level pressures of the pass are required beforehand
 * (i_reinterp = 1, step_03:202-216). */

/* step_03:192-193: delta_ps += adj_ps ; ps_pgw = PS + delta_ps.  PS, ps_pgw storage dtype (ntime,ncol);
 * delta_ps, adj_ps double. */
int pgw_update_ps(pgw_ctx *ctx, int dtype, long long n, const void *PS, double *delta_ps,
                  const double *adj_ps, void *ps_pgw);

/* phi_ref of a hybrid-level state (T, QV, PS, FIS) at scalar or per-column p_ref, fp64 output:
 * integ_geopot(ak + PS*bk, FIS, T, QV, ., p_ref) without the 4-D pressure array
 * (step_03:280-287 with :64-66). */
int pgw_phi_ref_hybrid(pgw_ctx *ctx, int dtype, int ntime, long long ncol, const void *T, const void *QV,
                       const void *PS, const void *FIS, double p_ref, const double *p_ref_field,
                       double *phi_ref);

/* a5 the whole loop step_03_apply_to_era.py:182-319 with its control flow: passes until
 * max|err| <= thresh; error when the pass counter exceeds max_n_iter (so at most
 * max_n_iter-1 passes succeed); the adj_ps of the last pass is NOT applied.
 *  T, QV: the ERA fields for phi_ref_era (computed once; it is constant for fixed p_ref);
 *  dzg_pref (ntime, ncol) storage dtype: zg delta [m] at plev == p_ref (multiplied by g here);
 *  outputs: ps_pgw (ntime, ncol), hus_pgw (ntime, nlev, ncol) storage dtype (either may be NULL),
 *  n_iter, max_err_hist[max_n_iter] (host, may be NULL). */
int pgw_adjust_ps_loop(pgw_ctx *ctx, int dtype, int ntime, long long ncol,
                       const void *PS, const void *FIS, const void *T, const void *QV,
                       const void *ta_pgw, const void *hur_pgw, const void *dzg_pref,
                       double p_ref, double adj_factor, double thresh, int max_n_iter,
                       void *ps_pgw, void *hus_pgw, int *n_iter, double *max_err_hist);

/* sum over columns and passes of the full levels the last pgw_adjust_ps_loop actually read
 * (the pass kernel stops a wave above p_ref); used for the bytes-moved accounting. */
unsigned long long pgw_last_levels_touched(pgw_ctx *ctx);

/* PGW_OPT_QV_FROM_PASS: 1 when the finalize kernel of the last pgw_adjust_ps_loop / pgw_step03_file took the QV below p_ref from
 * the converged pass (that pass was the last one of its launch), else 0.  *skipped (may be NULL): the level-columns of hus_pgw
 * the finalize kernel then left alone, summed over columns - it read e and wrote QV on the other
 * (nlev - qv_done_levels) * ntime * ncol - *skipped.  With PGW_OPT_FINISH_IN_PASS that pass has written them all and ps_pgw: no
 * finalize kernel ran, and *skipped is (nlev - qv_done_levels) * ntime * ncol. */
int pgw_last_qv_from_pass(pgw_ctx *ctx, unsigned long long *skipped);

/* ---------------------------------------------------------------- whole file ---------- */
/* The per-file compute path of pgw_for_era5 (reference step_03_apply_to_era.py:62-346 with
 * i_reinterp = 0 and a fixed p_ref) as ONE call on device-resident arrays, using fused kernels:
 *   ta+hur: RELHUM of the ERA state (:91-94), both delta interpolations incl. surface insertion
 *           (functions.py:306-431), the add (:170-173) and e = hur_pgw/100*e_sat(ta_pgw)
 *           (functions.py:123) in one pass over T, QV;
 *   ua+va : both delta interpolations + add in one pass over U, V;
 *   phi_ref of the ERA state from (T, QV, PS, FIS) without a 4-D pressure array (:280-287);
 *   the fixed-point loop (:182-319) and the final PS / QV (:193, :262-266, :369-371);
 *   the surface riders (:103-146).
 * All field pointers are device pointers in storage `dtype`; delta records are the two
 * bracketing time records (`*_a` may be NULL / x_hi == 0 for an exact hit, functions.py:282-283).
 * Results are identical to calling the function-level entry points in the reference's order. */
typedef struct pgw_file_args {
    /* shapes */
    int dtype, ntime, nlev, nplev, nsoil, ignore_top, max_n_iter;      /* 2 <= nplev <= 128 (PGW_MAX_PLEV) */
    int local_p_ref;      /* != 0: p_ref_inp = None, reference pressure chosen per column and pass (step_03:219-253) */
    int ref_dtype;        /* != 0 (dtype must be PGW_F32): reference-dtype mode - the float32 roundings numpy's promotion
                             puts into the reference on float32 ERA5 files are reproduced (phi_hl stored float32 per level,
                             functions.py:141,149; float32 tav of the ERA state :144; float32 delta_ps / ps_pgw,
                             step_03:182-193; float32 e_sat chain of RELHUM, functions.py:74-105) and, like the reference's
                             `era + delta` (step_03:170-173), the 4-D outputs T_out, QV_out, U_out, V_out (and hur_pgw_out)
                             are FLOAT64 arrays; PS_out and the surface riders stay float32.
                             0: float64 arithmetic on the stored values, outputs in `dtype`. */
    int _pad0;
    long long ncol;
    /* ERA5 file (device) + small host tables */
    const void *PS, *FIS, *T, *QV, *U, *V;                  /* (ntime,ncol) / (ntime,nlev,ncol)   */
    const void *T_SKIN, *T_SO, *FR_LAND, *FR_SEA_ICE;       /* surface riders, NULL to skip them  */
    const double *soil_depth;                               /* host, nsoil                        */
    const double *plev;                                     /* host, nplev, file order            */
    /* delta records (device) */
    const void *ta_b, *ta_a, *hur_b, *hur_a, *ua_b, *ua_a, *va_b, *va_a;   /* (ntime,nplev,ncol) */
    const void *zg_b, *zg_a;                                /* (ntime,ncol): zg delta at plev == p_ref */
    const void *zg3_b, *zg3_a;                              /* full zg records (local_p_ref): (ntime,nplev,ncol), or
                                                               (ntime,nplev_zg,ncol) when nplev_zg != 0 */
    const void *tas_b, *tas_a, *hurs_b, *hurs_a, *pshist_b, *pshist_a;     /* (ntime,ncol)       */
    const void *siconc_b, *siconc_a, *ts_b, *ts_a, *tos_b, *tos_a, *ts_clim;
    double x_hi, x_new;                                     /* time-lerp abscissae (pgw_time_lerp) */
    /* loop controls (settings.py:140-150 of the reference) */
    double p_ref, adj_factor, thresh;
    /* outputs (device); T_out..V_out (ntime,nlev,ncol); hur_pgw_out optional (may be NULL) */
    void *PS_out, *T_out, *QV_out, *U_out, *V_out, *hur_pgw_out;
    void *T_SKIN_out, *T_SO_out, *FR_SEA_ICE_out;
    /* results */
    int n_iter;
    int passes_launched;  /* passes executed, including passes speculated beyond convergence (multi-pass launches); with
                             PGW_OPT_FUSED_FIRST the first pass, which the delta kernel runs, counts as launched */
    unsigned long long levels_touched;   /* full levels read by the LOOP kernels' passes, summed over columns and passes up to the
                             converged one: with PGW_OPT_FUSED_FIRST pass 1 adds only the columns the delta kernel left to them */
    double max_err_hist[32];
    /* The reference loads every delta file on its own (load_delta, functions.py:195-303): files may have different time
     * axes - monthly tos / siconc beside daily 3-D deltas - so a variable's bracketing records and abscissae are its own.
     * per_var_time != 0: the records of zg, siconc, ts and tos are interpolated with the pairs below (x_hi == 0: the
     * instant is a record of that file, `_a` ignored); x_hi / x_new above remain the pair of ta, hur, ua, va, tas, hurs and
     * ps_hist, which the quad kernel interpolates together (a member of that group on another axis is handed over
     * already interpolated by the caller, `_a` == `_b`).  per_var_time == 0: one pair for all (x_hi / x_new). */
    int per_var_time;
    /* != 0: settings.i_reinterp = 1 (step_03_apply_to_era.py:202-216, 330-343) - in every pass of the loop the ERA ta / hur
     * fields and their deltas are interpolated onto the CURRENT model-level pressures, ua / va once after convergence;
     * fixed or local p_ref, every storage mode incl. ref_dtype.  One kernel sequence and one host read-back per pass
     * (the multi-pass loop kernel needs iterate-independent T_pgw / e); no latitude-band sharding. */
    int i_reinterp;
    double zg_x_hi, zg_x_new, siconc_x_hi, siconc_x_new, ts_x_hi, ts_x_new, tos_x_hi, tos_x_new;
    /* local_p_ref != 0 with zg on a plev axis of its own (the reference takes the candidates for the reference level from
     * zg's plev, step_03:219-222, and selects the zg delta on it, :292-295; in the CFday workflow ta / hur / ua / va stand
     * on 99 levels and zg on Emon / Amon's).  nplev_zg == 0: zg shares `plev` (then nplev <= 64).  Otherwise plev_zg
     * (host, nplev_zg, file order) is the axis of zg3_b / zg3_a and of the level search, in every form of the loop
     * (multi-pass, one launch per pass, i_reinterp).  1 <= nplev_zg <= 64 (PGW_MAX_PLEV_ZG): the loop kernel carries this
     * table by value and sits on its register budget; a zg file has 19 to 34 levels.  Ignored with a fixed p_ref. */
    int nplev_zg, _pad1;
    const double *plev_zg;
} pgw_file_args;

/* Who produces the loop's state (fixed p_ref, multi-pass loop).  With PGW_OPT_FUSED_FIRST = 1 the delta kernel, walking each
 * column from the surface up, integrates phi_ref of the ERA state and of the PGW state of pass 1 (delta_ps = 0: the same
 * half-level pressures) while the levels below p_ref are in its registers, and leaves phi_ref_era, dphi_clim, delta_ps = 0,
 * adj_ps, the first row of the delta_ps history and max |err| of pass 1 (status block of pass 1) - for every group of 64
 * columns whose half-level pressures all ascend (ps >= the smallest such ps of the level table; not NaN).  The other groups
 * are flagged; the first loop launch runs its own ERA-state scan and pass 1 for them alone and a continuation launch
 * passes 2 .. loop_guess for all columns.  With 0 the first loop launch does all of it, as pgw_adjust_ps_loop always does.
 * The two give the same bits, pass counts, histories and error reports. */
int pgw_step03_file(pgw_ctx *ctx, pgw_file_args *args);

/* The record bracketing of load_delta (functions.py:224-283) on integer seconds since 1970-01-01 - host arithmetic only,
 * no HIP call.  times_s[n]: the stamps of one delta file; target_s: the instant of the ERA5 file.
 *  - the LAST stamp that is a Feb 29 is dropped (:224-230): *dropped = its index, -1 when there is none;
 *  - every kept stamp is re-yeared to the target's year (:235-238): first second of (year, the stamp's month) + the stamp's
 *    offset within its month, so a remaining Feb 29 rolls into March in a non-leap year;
 *  - *ind_before = the last kept stamp <= target, *ind_after = the first kept stamp >= target (:242-243, :262-263), both as
 *    indices into the KEPT stamps (record index = i + (dropped >= 0 && i >= dropped)); when there is no stamp at or before
 *    the target the last kept stamp re-yeared to year - 1 stands in (:253-258), when there is none at or after it the first
 *    one re-yeared to year + 1 (:273-278);
 *  - *x_hi = (double)(after - before), *x_new = (double)(target - before) in nanoseconds, the int64 differences cast as
 *    Python's float(int) rounds them; both 0.0 when *ind_before == *ind_after (:282-283).
 * PGW_ERR_ARG: a NULL pointer, n < 1, or no stamp kept. */
int pgw_delta_bracket(const long long *times_s, int n, long long target_s, int *ind_before, int *ind_after, double *x_hi,
                      double *x_new, int *dropped);

/* What pgw_step03_file needs for a file, split into what stays from file to file and what the instant decides.  A plain
 * struct the caller owns and fills (the library keeps no copy and allocates nothing for it): ERA5 and output pointers, shapes,
 * tables and loop controls in `args`; for every delta variable whose record array is resident on the device, where its records
 * lie and which time axis brackets them.  pgw_step03_file_at then costs the host one call per file. */
#define PGW_PLAN_MAX_AXES 8
enum pgw_plan_var_id {
    PGW_PV_TA = 0, PGW_PV_HUR, PGW_PV_UA, PGW_PV_VA, PGW_PV_TAS, PGW_PV_HURS, PGW_PV_PS_HIST,   /* the quad group: ta's axis */
    PGW_PV_ZG, PGW_PV_SICONC, PGW_PV_TS, PGW_PV_TOS,                                           /* bracketed on their own */
    PGW_PV_COUNT
};
typedef struct pgw_plan_var {
    const void *base;          /* device, record 0 of the resident array [nrec, ...]; NULL: the template's pointers stay */
    long long rec_bytes;       /* bytes from one record to the next */
    long long ref_offset;      /* zg with a fixed p_ref: bytes from a record's start to its plev == p_ref slab; else 0 */
    int axis;                  /* index into axis_times */
    int _pad;
} pgw_plan_var;
typedef struct pgw_file_plan {
    pgw_file_args args;        /* template: every field that does not depend on the instant (per_var_time must be 1) */
    int n_axes, _pad;
    const long long *axis_times[PGW_PLAN_MAX_AXES];   /* host, seconds since 1970-01-01, one entry per distinct time axis */
    int axis_len[PGW_PLAN_MAX_AXES];
    pgw_plan_var var[PGW_PV_COUNT];
} pgw_file_plan;

/* pgw_step03_file for the instant `target_s`: *filled = plan->args; every axis bracketed once (pgw_delta_bracket); the `_b` /
 * `_a` record pointers of every variable with a base; x_hi / x_new from ta's axis (the whole quad group must share it);
 * zg_x_*, siconc_x_*, ts_x_*, tos_x_* from each variable's own; zg into zg3_b / zg3_a when args.local_p_ref, else zg_b / zg_a
 * at ref_offset; then pgw_step03_file(ctx, filled).  *filled carries the results (n_iter, max_err_hist, levels_touched,
 * passes_launched) and shows what the call was made with. */
int pgw_step03_file_at(pgw_ctx *ctx, const pgw_file_plan *plan, long long target_s, pgw_file_args *filled);

/* ---------------------------------------------------------------- step_02 regridding - */
/* a10 regrid_lat_lon, xarray branch (functions.py:774-789, 817-893): separable linear
 * interpolation, latitude first then longitude, on tables the host derives from the
 * coordinates (pole rows = zonal mean, periodic +-360 copies, scipy interp1d index rule).
 *  src (nfield, nlat_s, nlon_s); out (nfield, nlat_t, nlon_t);
 *  lat_lo/lat_hi (nlat_t): source row of the lower/upper neighbour in the EXTENDED ascending
 *    latitude axis: -1 = south-pole row, nlat_s = north-pole row, else physical row index
 *    (already un-flipped); lat_dx = x_new - x_lo, lat_Dx = x_hi - x_lo; lat_oob != 0 -> NaN.
 *  lon_lo/lon_hi (nlon_t): physical source column (periodic copies folded); lon_dx, lon_Dx, lon_oob.
 *  pole rows use the NaN-skipping zonal mean of physical row `south_row` / `north_row`.  Tables whose non-oob lat_lo /
 *  lat_hi entries name the south-pole row (-1) while south_row < 0, or the north-pole row (nlat_s) while north_row < 0, are
 *  rejected with PGW_ERR_ARG before anything is uploaded or launched. */
int pgw_regrid_bilinear(pgw_ctx *ctx, int dtype, long long nfield, int nlat_s, int nlon_s,
                        int nlat_t, int nlon_t, const void *src,
                        const int *lat_lo, const int *lat_hi, const double *lat_dx, const double *lat_Dx,
                        const int *lat_oob,
                        const int *lon_lo, const int *lon_hi, const double *lon_dx, const double *lon_Dx,
                        const int *lon_oob,
                        int south_row, int north_row, void *out);

/* The same regridding from a plan: the ten tables of one (source grid, target mesh) pair uploaded once into device memory the
 * plan owns, with the pole scratch for up to max_nfield planes - for a caller that regrids many records of one grid pair in
 * the middle of other work on the context's stream (step_03 with settings.delta_grid = 'source': a delta record is regridded
 * straight into its slot of the DeltaSet's window).
 *  pgw_regrid_plan_create: the ten tables HOST, as for pgw_regrid_bilinear and checked like them (shapes, null pointers, table
 *    entries, pole rows; max_nfield >= 1): PGW_ERR_ARG with *plan = NULL and nothing allocated.  Synchronises the stream once;
 *    the host tables may be freed after the call.
 *  pgw_regrid_plan_apply: src (nfield, nlat_s, nlon_s) of dtype_src, out (nfield, nlat_t, nlon_t) of dtype_out, both DEVICE.
 *    Every value is computed as pgw_regrid_bilinear computes it for dtype_src (the same kernel, the same bits) and rounded to
 *    dtype_src; where dtype_out differs, that value is then converted to dtype_out - what a file written by step_02 in the
 *    source's type holds after the host's astype(dtype_out).  Launches on the context's stream and returns: no allocation,
 *    no workspace slot, no synchronisation.  PGW_ERR_ARG before any launch, the output untouched, for: a null plan or pointer,
 *    a dtype tag other than PGW_F32 / PGW_F64, nfield outside [1, max_nfield], src or out not aligned to its element size.
 *    Timed under PGW_K_REGRID.
 *  pgw_regrid_plan_destroy: waits for the stream, frees the plan (NULL: nothing to do). */
typedef struct pgw_regrid_plan pgw_regrid_plan;
int pgw_regrid_plan_create(pgw_ctx *ctx, int nlat_s, int nlon_s, int nlat_t, int nlon_t,
                           const int *lat_lo, const int *lat_hi, const double *lat_dx, const double *lat_Dx,
                           const int *lat_oob,
                           const int *lon_lo, const int *lon_hi, const double *lon_dx, const double *lon_Dx,
                           const int *lon_oob,
                           int south_row, int north_row, long long max_nfield, pgw_regrid_plan **plan);
int pgw_regrid_plan_apply(pgw_ctx *ctx, const pgw_regrid_plan *plan, int dtype_src, int dtype_out, long long nfield,
                          const void *src, void *out);
int pgw_regrid_plan_destroy(pgw_ctx *ctx, pgw_regrid_plan *plan);

/* a10 with point-wise targets (functions.py:812-893 where `targ_lat` / `targ_lon` are 2-D over shared dimensions, or 1-D
 * over one shared dimension: `.interp({lat: targ_lat})` then `.interp({lon: targ_lon})` is xarray's point-wise
 * interpolation): every target g has its own latitude and its own longitude bracket.  Same arithmetic, same order and
 * the same pole values as pgw_regrid_bilinear - a mesh handed over as points gives the same bits.
 *  src (nfield, nlat_s, nlon_s) DEVICE; out (nfield, ntarg) DEVICE; the nine tables HOST, length ntarg, uploaded here:
 *  lat_lo / lat_hi / lat_dx / lat_Dx and lon_lo / lon_hi / lon_dx / lon_Dx as above, per target; oob != 0 (lat_oob | lon_oob)
 *  -> NaN, the target's other entries are not read.  A NaN dx (NaN target coordinate) or a NaN corner gives NaN.
 *  PGW_ERR_ARG before anything is uploaded or launched for: nfield < 1, ntarg < 1, a source grid below 2 x 2, a null
 *  pointer, a non-oob lat index outside [-1, nlat_s] or lon index outside [0, nlon_s), a pole row named while south_row /
 *  north_row < 0.  One target per lane.  Timed under PGW_K_REGRID. */
int pgw_regrid_points(pgw_ctx *ctx, int dtype, long long nfield, int nlat_s, int nlon_s, long long ntarg, const void *src,
                      const int *lat_lo, const int *lat_hi, const double *lat_dx, const double *lat_Dx,
                      const int *lon_lo, const int *lon_hi, const double *lon_dx, const double *lon_Dx,
                      const int *oob, int south_row, int north_row, void *out);

/* Winds on a rotated-pole target grid (not in the reference, whose targets are lat-lon meshes).  A file on a
 * `rotated_latitude_longitude` mapping stores GRID-RELATIVE components - U along increasing rlon, V along increasing rlat -
 * while the GCM's ua / va are eastward / northward.  At a target at geographic (lat, lon), the north pole of the rotated grid at
 * geographic (pole_lat, pole_lon) (CF grid_north_pole_latitude / grid_north_pole_longitude), all in degrees:
 *    D = pole_lon - lon;   a1 = cos(pole_lat) sin(D);   a2 = sin(pole_lat) cos(lat) - cos(pole_lat) sin(lat) cos(D)
 *    rho = sqrt(a1^2 + a2^2);   c = a2 / rho,  s = a1 / rho
 *    u_rot = u c - v s,  v_rot = u s + v c            inverse:  u = u_rot c + v_rot s,  v = -u_rot s + v_rot c
 * (COSMO's uv2uvrot).  All three run on the context's stream and are timed under PGW_K_REGRID; PGW_ERR_ARG before anything is
 * launched, the outputs untouched, for a null pointer, n < 1, nfield < 1 or an unknown dtype.
 *
 *  pgw_wind_rotation: cos_out[g] = c, sin_out[g] = s of the n targets (lat, lon); all arrays float64, DEVICE.  Sines and
 *    cosines are exact at multiples of 90 degrees, so a pole at (90, +-180) gives c = 1, s = 0.  rho == 0 (a pole of the
 *    rotated grid, where the direction is undefined) gives (1, 0); a NaN coordinate gives NaN in both.
 *  pgw_rotate_pair: u, v (nfield, n) of `dtype` -> u_out, v_out, the rotation by cos / sin (n, float64, DEVICE) in float64,
 *    each result rounded once to `dtype`; inverse != 0 rotates back.  In place when u_out == u and v_out == v.  16-byte
 *    accesses where n and the addresses allow, single elements otherwise: the same bits.
 *  pgw_regrid_points_wind: pgw_regrid_points on src_u and src_v (same arguments, checks and pole values, one set of tables)
 *    and the rotation by the targets' cos / sin (ntarg, float64, DEVICE) in one launch: u_out, v_out (nfield, ntarg) hold the
 *    bits of pgw_regrid_points on each component followed by pgw_rotate_pair - each regridded value is rounded to `dtype`
 *    before it is rotated.  An oob target gives NaN in both. */
int pgw_wind_rotation(pgw_ctx *ctx, long long n, const double *lat, const double *lon, double pole_lat, double pole_lon,
                      double *cos_out, double *sin_out);
int pgw_rotate_pair(pgw_ctx *ctx, int dtype, long long nfield, long long n, const void *u, const void *v, const double *cos,
                    const double *sin, int inverse, void *u_out, void *v_out);
int pgw_regrid_points_wind(pgw_ctx *ctx, int dtype, long long nfield, int nlat_s, int nlon_s, long long ntarg,
                           const void *src_u, const void *src_v,
                           const int *lat_lo, const int *lat_hi, const double *lat_dx, const double *lat_Dx,
                           const int *lon_lo, const int *lon_hi, const double *lon_dx, const double *lon_Dx,
                           const int *oob, int south_row, int north_row, const double *cos, const double *sin,
                           void *u_out, void *v_out);

/* The point-wise regridding from a plan: the nine tables of one (source grid, target list) pair, the targets' cos / sin where
 * the plan rotates, and the pole scratch for up to 2 * max_nfield planes (u and v), uploaded once into device memory the plan
 * owns - for a caller that regrids many records onto one list of targets in the middle of other work on the context's stream
 * (step_03 with settings.delta_grid = 'source_points': a delta record is regridded straight into its slot of the DeltaSet's
 * window, ua / va rotated onto a rotated-pole file's directions in the same launch).
 *  pgw_points_plan_create: the nine tables HOST, length ntarg, as for pgw_regrid_points and checked like them (shapes, null
 *    pointers, table entries, pole rows; max_nfield >= 1).  cos / sin (ntarg, float64, DEVICE, as pgw_wind_rotation writes
 *    them): both given - they are copied into the plan's memory on the stream - or both NULL: the plan cannot rotate.
 *    PGW_ERR_ARG with *plan = NULL and nothing allocated.  Synchronises the stream once; the host tables and cos / sin may be
 *    freed after the call.
 *  pgw_points_plan_apply: src (nfield, nlat_s, nlon_s) of dtype_src, out (nfield, ntarg) of dtype_out, both DEVICE.  Every
 *    value is computed as pgw_regrid_points computes it for dtype_src (the same kernel, the same bits) and rounded to dtype_src;
 *    where dtype_out differs, that value is then converted to dtype_out - what a file written by step_02 in the source's type
 *    holds after the host's astype(dtype_out).
 *  pgw_points_plan_apply_wind: src_u, src_v -> u_out, v_out likewise, as pgw_regrid_points_wind: each regridded component is
 *    rounded to dtype_src and rotated in float64, each result rounded once to dtype_src - what a `--rotate_winds` file of
 *    step_02 holds - and then converted to dtype_out.  The pole means are taken per component.
 *  Both launch on the context's stream and return: no allocation, no workspace slot, no synchronisation.  PGW_ERR_ARG before
 *    any launch, the outputs untouched, for: a null plan or pointer, a dtype tag other than PGW_F32 / PGW_F64, nfield outside
 *    [1, max_nfield], a pointer not aligned to its element size, apply_wind on a plan made without cos / sin.  Timed under
 *    PGW_K_REGRID.
 *  pgw_points_plan_destroy: waits for the stream, frees the plan (NULL: nothing to do). */
typedef struct pgw_points_plan pgw_points_plan;
int pgw_points_plan_create(pgw_ctx *ctx, int nlat_s, int nlon_s, long long ntarg,
                           const int *lat_lo, const int *lat_hi, const double *lat_dx, const double *lat_Dx,
                           const int *lon_lo, const int *lon_hi, const double *lon_dx, const double *lon_Dx,
                           const int *oob, int south_row, int north_row, long long max_nfield,
                           const double *cos, const double *sin, pgw_points_plan **plan);
int pgw_points_plan_apply(pgw_ctx *ctx, const pgw_points_plan *plan, int dtype_src, int dtype_out, long long nfield,
                          const void *src, void *out);
int pgw_points_plan_apply_wind(pgw_ctx *ctx, const pgw_points_plan *plan, int dtype_src, int dtype_out, long long nfield,
                               const void *src_u, const void *src_v, void *u_out, void *v_out);
int pgw_points_plan_destroy(pgw_ctx *ctx, pgw_points_plan *plan);

/* regrid_lat_lon, xESMF branch (functions.py:797-810, settings.py:117-129): what `xe.Regridder(ds_in, ds_era5, "bilinear",
 * periodic=periodic_lon)` (:799-800) asks ESMF for and `regridder(ds_in[var_name])` (:802) applies, for source grids with
 * 2-D coordinates (rotated-pole, curvilinear).  Bilinear on the unit sphere in 3-D Cartesian space, cell edges being chords;
 * the definition (patch, Newton solve, Cramer order, tolerances, pole caps, lowest accepting cell) is written out above
 * k_cell_locate in pgw4era5_amd/csrc/pgw_kernels.h and restated in numpy in tests/test_regrid_curvilinear_host.py.  Parity
 * with ESMF itself is unpinned.  PRECONDITIONS: cells are convex and smaller than a hemisphere; concave
 * cells are not detected.  All pointers are DEVICE pointers except n_unmapped.
 *
 * Locate (:799-800), once per grid pair.  P (ntarg, 3): target unit vectors.  X (ny*nx, 3), or (ny*nx + 2, 3) when
 * periodic: source node unit vectors (cos lat cos lon, cos lat sin lon, sin lat), formed by the caller; when periodic, the
 * two appended vectors are the poles of the caps, normalise(sum_i X[je, i]) of row je = 0 and of row ny - 1.  Buckets: a
 * uniform nb^3 grid over [-1, 1]^3, bucket id = (bx * nb + by) * nb + bz with b = clamp((int)((x + 1) * 0.5 * nb), 0, nb - 1);
 * bucket_start (nb^3 + 1), bucket_cells: per bucket, ASCENDING, every cell whose bounding box - enlarged by the radial bulge
 * of its patch and the acceptance tolerance - touches it (pgw4era5_amd.functions.curvilinear_buckets).  Cells: quads
 * j * ncx + i (ncx = nx when periodic, else nx - 1), then the nx cap triangles of row 0 and those of row ny - 1 (periodic
 * only).  Results: idx (ntarg, 4) source node of each entry, -1 = absent (never read), ny*nx / ny*nx + 1 = the pole nodes;
 * w (ntarg, 4); *n_unmapped = targets no cell accepts (four -1).  Synchronous. */
int pgw_bilinear_locate(pgw_ctx *ctx, long long ntarg, const double *P, int ny, int nx, int periodic, const double *X,
                        int nb, const int *bucket_start, const int *bucket_cells, int *idx, double *w,
                        long long *n_unmapped);

/* Apply (:802).  src (nfield, ny, nx), out (nfield, ntarg) in `dtype`; out[f, g] = w0*v0, then + wk*vk over the present
 * entries in order, in float64 on the stored values, stored in `dtype`; NaN in a present entry gives NaN (xESMF
 * skipna=False); an unmapped target gets 0.0 (xESMF 0.6.2, environment.yml:177), NaN with unmapped_nan != 0.  A pole node's
 * value is the plain mean of its row, (sum_i v[je, i]) / nx in index order, NaN propagating.  Entries outside
 * [-1, ny*nx + 2) count as absent. */
int pgw_regrid_sparse(pgw_ctx *ctx, int dtype, long long nfield, int ny, int nx, long long ntarg, const void *src,
                      const int *idx, const double *w, int unmapped_nan, void *out);

/* Apply on the winds of a rotated-pole SOURCE grid (not in the reference): src_u, src_v (nfield, ny, nx) of `dtype` are
 * GRID-RELATIVE (U along rlon, V along rlat of the source grid) where src_cos / src_sin (ny*nx, float64, DEVICE, as
 * pgw_wind_rotation writes them for the source nodes and the source grid's pole) are given, and u_out, v_out (nfield, ntarg)
 * follow the targets' rotated grid where targ_cos / targ_sin (ntarg, DEVICE) are given.  The definition is the composed form
 *    ug, vg = pgw_rotate_pair(src_u, src_v, src_cos, src_sin, inverse = 1)       left out when src_cos = src_sin = NULL
 *    ur, vr = pgw_regrid_sparse(ug), pgw_regrid_sparse(vg)
 *    u,  v  = pgw_rotate_pair(ur, vr, targ_cos, targ_sin, inverse = 0)           left out when targ_cos = targ_sin = NULL
 * and the outputs hold its bits: each geographic source value is rounded to `dtype` before it is weighted, each regridded
 * value is rounded to `dtype` before it is rotated; a pole node's value is the plain index-order mean of the geographic,
 * rounded edge row, NaN propagating; an unmapped target's 0.0 (NaN with unmapped_nan != 0) goes through the target rotation
 * like any other value; absent entries stay unread.  Both pairs NULL: pgw_regrid_sparse on each component.
 * pgw_regrid_sparse's checks, and PGW_ERR_ARG before anything is launched, both outputs untouched, for: one pointer of a
 * cos / sin pair NULL and the other not, a pointer not aligned to its element, an output that overlaps an input or the other
 * output.  Runs on the context's stream, timed under PGW_K_REGRID_SPARSE. */
int pgw_regrid_sparse_wind(pgw_ctx *ctx, int dtype, long long nfield, int ny, int nx, long long ntarg,
                           const void *src_u, const void *src_v, const double *src_cos, const double *src_sin,
                           const int *idx, const double *w, int unmapped_nan,
                           const double *targ_cos, const double *targ_sin, void *u_out, void *v_out);

/* ---------------------------------------------------------------- surface riders ----- */
/* a9 step_03_apply_to_era.py:103-146 + integrate_tos functions.py:1145-1186, 2-D fields (n = ntime*ncol)
 *  sic_out = clip(sic + dsic/100, 0, 1)
 *  dts_comb = integrate_tos(dtos, dts, land, sic_out) ; tskin_out = tskin + dts_comb
 *  tso_out[s] = tso[s] + clim + exp(-soil_depth[s]/2.8)*(dts_comb - clim)   (nsoil levels) */
int pgw_surface_update(pgw_ctx *ctx, int dtype, int ntime, long long ncol, int nsoil,
                       const double *soil_depth,
                       const void *sic, const void *dsic, const void *dtos, const void *dts,
                       const void *land, const void *ts_clim, const void *tskin, const void *tso,
                       void *sic_out, void *dts_comb_out, void *tskin_out, void *tso_out);

/* ---------------------------------------------------------------- debug mode --------- */
/* step_03 --debug_mode interpolate_full (step_03_apply_to_era.py:350-361): the deltas the reference writes instead of the
 * ERA5 file, as arrays.  Both entries are synchronous function-level calls beside the whole-file entry; the whole-file entry
 * does not use them.
 *
 * The four deltas of load_delta_interp (functions.py:306-340) on the model-level pressures akm + ps*bkm (tables of
 * the last set_levels call), one kernel: the values the whole-file entry adds to T, RELHUM, U, V, with its
 * expressions (time interpolation of the records, surface insertion for ta / hur from tas / hurs / ps_hist, the column
 * interpolation in ln p), so `era + delta` in numpy reproduces its outputs bit for bit.  Records (ntime, nplev, ncol; 2 <= nplev <= 128) /
 * (ntime, ncol) in `dtype`, `*_a` unused when x_hi == 0 (the instant is a record); ps in `dtype`: PS of the file, or the
 * converged ps_pgw under settings.i_reinterp = 1 (step_03:212-216, 336-343).  ref_dtype = 1 (dtype PGW_F32 only): the
 * reference's dtype flow on float32 files.  Outputs (ntime, nlev, ncol) are float64 for every dtype
 * (xr.zeros_like(targ_P), functions.py:472-473).  Status codes and error columns as vert_interp_delta reports them for ta / hur:
 * PGW_ERR_PS_HIST_ABOVE_TOP (ps_hist not above min(plev), or NaN), PGW_ERR_TOP_PRESSURE unless ignore_top; target levels
 * that do not ascend restart the scan as there. */
int pgw_delta_fields(pgw_ctx *ctx, int dtype, int ref_dtype, int ntime, int nlev, int nplev, long long ncol,
                     const double *plev, const void *ps,
                     const void *ta_b, const void *ta_a, const void *hur_b, const void *hur_a,
                     const void *ua_b, const void *ua_a, const void *va_b, const void *va_a,
                     const void *tas_b, const void *tas_a, const void *hurs_b, const void *hurs_a,
                     const void *pshist_b, const void *pshist_a, double x_hi, double x_new, int ignore_top,
                     double *dta, double *dhur, double *dua, double *dva);

/* delta_ts_combined = integrate_tos(delta_tos, delta_ts, land, clip(sic + delta_siconc/100, 0, 1) of time 0)
 * (step_03:103-125) and delta_soilt[s] = clim + exp(-soil_depth[s]/2.8) * (delta_ts_combined - clim) (:139-143), float64
 * (ntime, ncol) and (ntime, nsoil, ncol); delta_soilt may be NULL.  The three 2-D deltas come as record pairs, each with the
 * abscissae of its own time axis, and are interpolated in the kernel as the whole-file entry does. */
int pgw_surface_deltas(pgw_ctx *ctx, int dtype, int ref_dtype, int ntime, long long ncol, int nsoil,
                       const double *soil_depth, const void *sic,
                       const void *siconc_b, const void *siconc_a, double siconc_x_hi, double siconc_x_new,
                       const void *tos_b, const void *tos_a, double tos_x_hi, double tos_x_new,
                       const void *ts_b, const void *ts_a, double ts_x_hi, double ts_x_new,
                       const void *land, const void *ts_clim, double *dts_comb, double *delta_soilt);

/* Spectral smoothing of a daily annual cycle, step_02 `smoothing`: filter_data / harmonic_ac_analysis,
 * functions.py:603-740.  in / out: (ntime, inner) C-order, inner = product of the non-time dimensions; every
 * column's series is replaced by mean + its first three harmonics (Storch & Zwiers 12.19-12.23), all NaN if the
 * series holds a NaN (:694-696).  cos_tab / sin_tab: host tables [3][ntime] of cos / sin(2*pi*i/ntime * t), t = 1..ntime,
 * i = 1..3, evaluated by the caller as the reference does (:716, 727).  ntime < 8 -> PGW_ERR_ARG with the reference's
 * message (:734-737); ntime <= 1365. */
int pgw_harmonic_smooth(pgw_ctx *ctx, int dtype, int ntime, long long inner, const double *cos_tab,
                        const double *sin_tab, const void *in, void *out);

/* NaN-ignoring Gaussian-kernel interpolation of a point cloud onto target points, step_02 for tos / siconc:
 * nan_ignoring_interp, functions.py:900-1060 (pyvista PolyData.interpolate = VTK vtkPointInterpolator + vtkGaussianKernel,
 * radius footprint, null value NaN).  All pointers are DEVICE pointers, coordinates planar metres (functions.py:958-1023;
 * host side: pgw4era5_amd/geodesy.py).
 *  tx, ty (ntarg): target points.  sx, sy (nsrc), sval (nsrc, nfield): source points SORTED by cell of a uniform grid of
 *  square cells (edge `cell` >= radius, origin (x0, y0), ncx x ncy cells, cell id = ix * ncy + iy), `cell_start`
 *  (ncx*ncy + 1 ints): first point of each cell.  sval may hold NaN: that point is skipped for that field (month).
 *  out (nfield, ntarg): sum_i w_i v_i / sum_i w_i, w_i = exp(-(sharpness/radius)^2 d_i^2) over the points with
 *  d_i <= radius; the value of a coincident point (d^2 < 256 eps); NaN where no point lies within the radius. */
int pgw_gauss_interp(pgw_ctx *ctx, long long ntarg, const double *tx, const double *ty, int ncx, int ncy,
                     double x0, double y0, double cell, const int *cell_start, long long nsrc, const double *sx,
                     const double *sy, const double *sval, int nfield, double radius, double sharpness, double *out);

/* The planar "metre" coordinates of that interpolation (functions.py:958-975, 1010-1023: per point three
 * pyproj.Geod(ellps="WGS84").inv lengths - the meridian arc from the equator, the geodesic between (0, lat) and
 * (lon, lat), and the one between (0, lat) and (180, lat)) for n points: lat, lon [deg], lon in (-180, 180]; outputs
 * lat_m = sign(lat) * arc, lon_m = sign(lon) * geodesic, lon_off = over-the-pole length [m].  Device pointers.  Vincenty's
 * series arranged as in pgw4era5_amd/geodesy.py (bisection on the departure azimuth; no iteration that can fail). */
int pgw_planar_metres(pgw_ctx *ctx, long long n, const double *lat, const double *lon, double *lat_m, double *lon_m,
                      double *lon_off);

/* Target side of that interpolation for POINT-WISE targets (2-D lat / lon of a rotated-pole file, a cell list;
 * functions.py:998-1023 without the mesh).  pgw_ocean_targets: lat, lon [deg] of n targets -> planar metres tx, ty; a longitude
 * above 180 is folded by -360; the lengths are evaluated on (|lat|, |lon|) and multiplied by sign(lat), sign(lon), as the
 * mesh path does for the distinct values of its axes (same device code as pgw_planar_metres: same bits).  `land` (n, may be
 * NULL): a target with land > 0.7 (:1032; a NaN fraction is not) or a NaN coordinate is inactive, tx = ty = NaN.
 * pgw_gauss_interp_points: pgw_gauss_interp for targets in any order (NaN coordinates = inactive); the library orders them
 * by the cell of the source grid they fall into (key, counting sort, scatter - all on the device, workspace of the context)
 * and walks blocks of 256 sorted targets; out (nfield, ntarg) in the CALLER's order, every element written, inactive targets
 * NaN.  Bit for bit what pgw_gauss_interp gives for the same (tx, ty), whatever the order.  A target outside the cell grid
 * is treated like one in the ring of cells around it (it can be within one radius of a border cell's points); ntarg < 2^31
 * and 16 * (ncx + 2) * (ncy + 2) < 2^31.  The walk is timed under PGW_K_GAUSS_INTERP; key and order are not profiled
 * separately (pgw_timer_start / _stop around the call gives the sum).  Device pointers. */
int pgw_ocean_targets(pgw_ctx *ctx, long long n, const double *lat, const double *lon, const double *land, double *tx,
                      double *ty);
int pgw_gauss_interp_points(pgw_ctx *ctx, long long ntarg, const double *tx, const double *ty, int ncx, int ncy,
                            double x0, double y0, double cell, const int *cell_start, long long nsrc, const double *sx,
                            const double *sy, const double *sval, int nfield, double radius, double sharpness, double *out);

/* Placement of the level arrays in HBM (no counterpart in the reference: numpy arrays live wherever malloc put them).
 * On an MI355X the rate a column kernel gets depends on WHERE hipMalloc put its arrays relative to each other: an array
 * written while an array of the same stretch of physical memory is read runs at 5.0-5.4 TB/s, arrays of different stretches
 * at 5.7-6.2.  pgw_placement_probe measures it for a given set: the column kernels' access pattern
 * with no arithmetic over n_src (0..4) read streams and n_dst (0..4) write streams of rows x ncol float64 each, `reps`
 * timed launches after one warm-up, *gbps = bytes moved / time.  The dst arrays are OVERWRITTEN.  Synchronous.
 * pgw_ws_adopt hands the library a pgw_malloc'ed buffer as its workspace `slot` (0 = the vapour-pressure field of the
 * file path, one ERA5 level field of float64) so that the host layer can choose that array's place too; the library owns
 * and frees it from then on; (NULL, 0) releases the slot. */
int pgw_placement_probe(pgw_ctx *ctx, int n_src, const void *const *src, int n_dst, void *const *dst, long long rows,
                        long long ncol, int reps, double *gbps);
int pgw_ws_adopt(pgw_ctx *ctx, int slot, void *dptr, size_t bytes);

/* Byte-order conversion on the device: dst[i] = byte-reversed src[i] for n elements of 4 or 8 bytes (in place
 * allowed).  NetCDF classic files are big-endian (the reference reads / writes them through xarray,
 * step_03_apply_to_era.py:60, 378, which converts on the host); with this entry the raw file bytes are uploaded
 * and converted at HBM speed, and results are converted before the download, so no host pass touches the fields. */
int pgw_byteswap(pgw_ctx *ctx, int elem_bytes, long long n, const void *src, void *dst);

/* dst[i] = (float)src[i], optionally written byte-reversed (big_endian != 0: the NetCDF classic byte order), n elements,
 * device pointers.  On float32 ERA5 files the reference's `era + delta` promotes T, QV, U, V to float64 and writes them
 * so (step_03_apply_to_era.py:170-173, 369-378: the output file is twice the input).  With settings.f32_out_dtype =
 * 'float32' the file driver computes exactly the same float64 fields and narrows them here on the way out - half the
 * download and half the file; values = the reference's, rounded once to float32.  No reference counterpart. */
int pgw_narrow_f64_f32(pgw_ctx *ctx, long long n, const double *src, void *dst, int big_endian);

/* diagnostic: out[i] = ln(in[i]) with the device logarithm every kernel uses (pgw_device.h
 * pgw_log: fdlibm log kernel for positive normal finite x, ocml log otherwise); device fp64 arrays */
int pgw_test_log(pgw_ctx *ctx, long long n, const double *in, double *out);
/* same for the table-driven logarithm of the hybrid-level loops (pgw_device.h pgw_log_tab: 128-entry table, r = fma(z, 1/c, -1),
 * degree-7 polynomial; generated by tools/gen_log_table.py) */
int pgw_test_log_table(pgw_ctx *ctx, long long n, const double *in, double *out);
/* same for pgw_log_f3 (pgw_log with three-address FMA Horner steps: the same bits) and pgw_log_dd (the fdlibm kernel carried
 * in double-double pairs: the logarithm whose last bit reaches a float64 result of integ_geopot in the reference's dtype flow) */
int pgw_test_log_f3(pgw_ctx *ctx, long long n, const double *in, double *out);
int pgw_test_log_dd(pgw_ctx *ctx, long long n, const double *in, double *out);

/* diagnostic: out[i] = pgw_exp(in[i]) (pgw_device.h: the device library's exp arithmetic written with explicit FMAs, the
 * exponential of every e_sat evaluation), ref[i] = exp(in[i]) of the device library; device fp64 arrays.  Tests require
 * out == ref bit for bit and <= 1 ulp from numpy. */
int pgw_test_exp(pgw_ctx *ctx, long long n, const double *in, double *out, double *ref);
/* diagnostic: out[i] = pgw_exp_finite(in[i]) (pgw_exp without the two range selects, with a guard on the remainder for huge
 * arguments); device fp64 arrays.  Tests require the bits of pgw_exp for every finite argument and NaN, and NaN at +-inf. */
int pgw_test_exp_finite(pgw_ctx *ctx, long long n, const double *in, double *out);
/* diagnostic: out[i] = pgw_exp_reduced(in[i]) (the same without that guard: the exponential of the float64 e_sat fast path and
 * of the Magnus formula of step_01, for |x| <= 1000); device fp64 arrays.  Tests require the bits of pgw_exp on that range. */
int pgw_test_exp_reduced(pgw_ctx *ctx, long long n, const double *in, double *out);

/* diagnostic: RELHUM of a float32 ERA state as numpy's promotion evaluates functions.py:58-116 on float32 files
 * (reference-dtype mode, step_03_apply_to_era.py:91-94): out = the form the quad kernel uses (the one phase a temperature
 * needs, scale-free divisions, expf without range selects), lit = the expression as written (both phases, IEEE divisions,
 * library expf); es / es_lit = the float32 e_sat alone.  hus, ta float32, pa float64; device arrays.  Tests require
 * out == lit and es == es_lit bit for bit over the physical range and the same special values outside it. */
int pgw_test_rh_f32(pgw_ctx *ctx, long long n, const float *hus, const double *pa, const float *ta,
                    double *out, double *lit, float *es, float *es_lit);

/* diagnostic: out[i] = num[i] / den[i] through the shared-divisor path (pgw_device.h SharedDivisor: reciprocal once,
 * three instructions per quotient) that the regridding and delta kernels use where many numerators share a divisor;
 * device fp64 arrays.  Tests require the IEEE quotient bit for bit. */
int pgw_test_shared_div(pgw_ctx *ctx, long long n, const double *num, const double *den, double *out);

/* integrate_tos(tos_field, ts_field, land_frac, ice_frac)  functions.py:1145-1186, flat over n */
int pgw_integrate_tos(pgw_ctx *ctx, int dtype, long long n, const void *tos, const void *ts,
                      const void *land, const void *ice, void *out);

/* ---------------------------------------------------------------- reference dtype flow, function level ---- */
/* settings.function_dtype_flow = 'reference' of pgw4era5_amd/functions.py.  The entries above take ONE `dtype` for all
 * operands and compute in fp64.  These take one dtype tag (PGW_F32 / PGW_F64) PER OPERAND, read every operand in its own
 * storage type and reproduce numpy's promotion through the cited reference lines: a python-float constant takes the type of
 * the array it meets, float32 (op) float32 is ONE IEEE float32 operation (-ffp-contract=off), float32 (op) float64 is
 * float64.  Only expf and the fp64 logarithm are not numpy's last bit.  Results have the dtype the reference returns.
 * A float32 pressure operand (pa_hl, a p_ref field, source / target pressures: the reference would take a float32
 * logarithm) and any other combination that is not instantiated: PGW_ERR_ARG with a message.  Data errors and their
 * codes as in the uniform entries. */

/* integ_geopot, functions.py:128-189: phi_hl rounded to the dtype of zgs at every level (:141, :149-152),
 * tav = ta*(1+0.61*hus) and CON_RD*tav in the promoted type of (ta, hus) (:144, :150), logarithms and the final expression
 * (:174-179) float64.  pa_hl and p_ref_field (may be NULL) float64 (dt_pa_hl = PGW_F64), phi_ref float64. */
int pgw_integ_geopot_mixed(pgw_ctx *ctx, int dt_pa_hl, int dt_zgs, int dt_ta, int dt_hus, int ntime, int nlev,
                           long long ncol, const void *pa_hl, const void *zgs, const void *ta, const void *hus,
                           double p_ref, const void *p_ref_field, double *phi_ref, int full_column);

/* The humidity functions, functions.py:58-125, the expression in numpy's promoted type at every node, e_sat and alpha wholly
 * in the type of ta.  which: 0 q -> e (a = hus, b = pa; :58-64), 1 e -> q (a = vapp, b = pa; :66-72), 2 / 3 e_sat over
 * water / ice (a = ta; :74-89), 4 mixed-phase e_sat (a = ta; :91-105), 5 q -> RH (a = hus, b = pa, c = ta; :107-116),
 * 6 RH -> q (a = hur, b = pa, c = ta; :118-125).  Operands a function does not take: NULL, tag ignored.  `out` has the
 * promoted type of the operands the function takes. */
int pgw_humidity_mixed(pgw_ctx *ctx, int which, int dt_a, int dt_b, int dt_c, long long n, const void *a,
                       const void *b, const void *c, void *out);

/* interp_logp_4d / interp_1d_for_timelatlon / interp_extrap_1d, functions.py:434-580: `src_y[i2] - src_y[i1]` in the
 * dtype of var (:575-578), everything else float64; all four `extrapolate` modes.  Pressures float64 (dt_p = PGW_F64),
 * out float64.  Other arguments as pgw_interp_logp_4d. */
int pgw_interp_logp_4d_mixed(pgw_ctx *ctx, int dt_var, int dt_p, int ntime, int nsrc, int ntarg, long long ncol,
                             const void *var, const void *source_P, const void *targ_P, int extrapolate,
                             int logp_in, double *out);

/* vert_interp_delta, functions.py:369-431 (+ :343-366): delta_sfc stored in the delta's dtype, ps_hist inserted into the
 * float64 source pressures, then as interp_logp_4d with 'constant'; `add_to` (may be NULL) is added in float64.
 * delta (ntime, nplev, ncol) in file order, 2 <= nplev <= 128; delta_sfc, ps_hist (ntime, ncol), both or neither; targ_P (ntime, nlev_t, ncol)
 * float64 (dt_targ = PGW_F64); out float64.  No time interpolation and no hybrid-level targets in this entry. */
int pgw_vert_interp_delta_mixed(pgw_ctx *ctx, int dt_delta, int dt_sfc, int dt_pshist, int dt_targ, int dt_add,
                                int ntime, int nplev, int nlev_t, long long ncol, const double *plev,
                                const void *delta, const void *delta_sfc, const void *ps_hist, const void *targ_P,
                                int ignore_top, const void *add_to, double *out);

/* replace_delta_sfc, functions.py:343-366: out_P float64, out_delta in the delta's dtype (np.vectorize allocates its
 * outputs from the first call's dtypes).  Other arguments as pgw_replace_delta_sfc. */
int pgw_replace_delta_sfc_mixed(pgw_ctx *ctx, int dt_delta, int dt_sfc, int dt_pshist, int ntime, int nplev,
                                long long ncol, const double *plev_asc, const void *delta, const void *delta_sfc,
                                const void *ps_hist, double *out_P, void *out_delta);

/* time interpolation of load_delta, functions.py:288-292 (scipy interp1d._call_linear): v_after - v_before in the promoted
 * type of the two records, slope and result float64. */
int pgw_time_lerp_mixed(pgw_ctx *ctx, int dt_before, int dt_after, long long n, const void *v_before,
                        const void *v_after, double x_hi, double x_new, double *out);

/* integrate_tos, functions.py:1145-1186: the blend (:1183-1184) in the operands' promoted type at every node, written into
 * the float64 array of :1180. */
int pgw_integrate_tos_mixed(pgw_ctx *ctx, int dt_tos, int dt_ts, int dt_land, int dt_ice, long long n,
                            const void *tos, const void *ts, const void *land, const void *ice, double *out);

/* ---------------------------------------------------------------- step_01 ------------ */
/* s1 model levels -> fixed pressure levels, fused       step_01_extract_deltas/CFday_interp_to_plev.py:89-134
 * = interp_logp_4d(var, ap + b * ps, targ_plev broadcast to every column, extrapolate) for one block of time steps,
 * without either 4-D pressure field: the source pressure ap[k] + b[k] * ps (:91) is formed per column in registers,
 * the logarithms of the one target list are taken once per thread block.
 *  var (ntime, nsrc, ncol), ps (ntime, ncol): device arrays of dtype_in; out (ntime, ntarg, ncol): device, dtype_out.
 *  ap, b (nsrc), targ_plev (ntarg): HOST arrays; nsrc in [2, 256], ntarg in [1, 256].
 *  src_reversed != 0: var, ap, b are stored with pressure DESCENDING along the level axis (surface first) and are read in
 *    reverse, which is the reference's reindex of :89; the kernel requires ascending source pressure like
 *    functions.py:500-501 (PGW_ERR_SRC_NOT_ASCENDING).  targ_plev is given ascending (np.sort, :114;
 *    PGW_ERR_TARG_NOT_ASCENDING when its last logarithm is below its first, functions.py:502-503); a list that is not
 *    monotone in between is served like interp_extrap_1d serves it.
 *  out_reversed != 0: row l of out holds target ntarg - 1 - l (pressure descending, :133-134).
 *  extrapolate: enum pgw_extrap; 'off' reports PGW_ERR_EXTRAP_OFF with the smallest offending column (pgw_error_column).
 *  dtype pairs: F32 -> F64 is the reference's dtype flow on float32 files (source pressure float64, src_y[i2] - src_y[i1]
 *    taken in float32 as numba does at functions.py:575-578, everything else and the result float64); F64 -> F64 is
 *    plain float64; F32 -> F32 is float64 arithmetic narrowed on the store (half the output; NOT the reference's bits).
 *    F64 -> F32 is not offered. */
int pgw_interp_hybrid_to_plev(pgw_ctx *ctx, int dtype_in, int dtype_out, int ntime, int nsrc, int ntarg, long long ncol,
                              const void *var, const void *ps, const double *ap, const double *b,
                              const double *targ_plev, int extrapolate, int src_reversed, int out_reversed, void *out);

/* s2 specific_to_relative_humidity(QV, P, T) of step_01_extract_deltas/Emon_convert_hus_to_hur.py:16-21 (a Magnus
 * formula; NOT the IFS formulas of functions.py:107-116):
 *   RH = 0.263 * P * QV * (exp(17.67 * (T - 273.15) / (T - 29.65)))**(-1)
 * qv, ta (ntime, nplev, ncol) device arrays of `dtype`; plev (nplev) HOST array, the pressure of each level (:53-55 make a
 * 4-D array of it; none exists here); rh (ntime, nplev, ncol) device, ALWAYS float64: on float32 files numpy evaluates
 * the exponent, exp and the reciprocal in float32 and the three-factor product in float64 (P is float64). */
int pgw_magnus_rh(pgw_ctx *ctx, int dtype, int ntime, int nplev, long long ncol, const void *qv, const double *plev,
                  const void *ta, double *rh);

/* s3 the coarse Amon hur carried onto the finer Emon levels     Emon_convert_hus_to_hur.py:82-122
 * hur (ntime, nplev, ncol) float64: the computed Emon field; amon (ntime, namon, ncol) of dtype_amon; out like hur.
 * Level table (HOST int arrays of length nplev, made by the caller from the two plev coordinates): copy_from[l] >= 0:
 * out level l = amon level copy_from[l] as it is (:122); otherwise (:85-118)
 *   a = |hur[l] - hur[e_above[l]]|, b = |hur[l] - hur[e_below[l]]|, w_above = 1 - a / (a + b), w_below = 1 - b / (a + b),
 *   out = amon[a_above[l]] * w_above + amon[a_below[l]] * w_below        (float64, this order; 0 / 0 = NaN is kept). */
int pgw_hur_merge_levels(pgw_ctx *ctx, int dtype_amon, int ntime, int nplev, int namon, long long ncol, const double *hur,
                         const void *amon, const int *copy_from, const int *e_above, const int *e_below,
                         const int *a_above, const int *a_below, double *out);

/* s4 multi-year mean of the records of one calendar bin  step_01_extract_deltas/extract_climate_delta.sh:153-159, 217-219
 * (`cdo ymonmean` / `cdo ydaymean` of the `-selyear` series; run a second time on the computed hur series, :235-238).
 * x (nrec, inner): device array of dtype_in, the bin's records in time order, NaN = missing value.  Per cell i, in record
 * order:  if (!isnan(x[r][i])) { sum += (double)x[r][i]; cnt += 1; }  - the sequential float64 sum, bit for bit.
 *  first != 0: start from zero, sum / cnt are not read; otherwise continue from sum (inner) float64 and cnt (inner) int32.
 *  last != 0: write mean[i] = (dtype_out)(sum / cnt), NaN where cnt == 0 (IEEE division), and NO state; otherwise write
 *    sum and cnt back and leave mean alone.
 *  With both set sum and cnt may be NULL and no accumulator exists in memory (a day-of-year bin of 30 years is one launch
 *  over 30 records); a month bin of daily data goes through in chunks that carry the state.
 *  dtype_out: dtype_in, or PGW_F64 for PGW_F32 input.  cdo's mean skips missing values the same way; parity with cdo's
 *  own summation order is not pinned (kind U). */
int pgw_clim_accumulate(pgw_ctx *ctx, int dtype_in, int dtype_out, int nrec, long long inner, const void *x, int first,
                        int last, double *sum, int *cnt, void *mean);

/* p1 T_CL of a COSMO extpar file + the time mean of the ts delta            postproc_cosmo/extpar_adapt.py:20-32
 *   delta_ts_clim = delta_ts.mean(dim=['time'])            - xarray on a float array: np.nanmean(values, axis=0)
 *   ext_file['T_CL'][:] += delta_ts_clim.values.squeeze()  - numpy's in-place add on netCDF4's masked array
 * x (nrec, n): device array of dtype_x (X), the records in time order, NaN = missing; base, out (n) of dtype_base (B).
 * Per cell i:
 *  1. x'[r] = isnan(x[r][i]) ? +0.0 : x[r][i];  tot = +0.0, then tot = (X)(tot + x'[r]) for r = 0 .. nrec - 1 in record
 *     order, in X (numpy's sum over the leading axis, which starts from the identity +0.0);  cnt = number of non-NaN
 *     records.  A NaN record ADDS +0.0.  Only a cell whose records are all -0.0 shows either: it sums to +0.0, with or
 *     without a NaN record, as numpy's does.
 *  2. mean = (X)((double)tot / (double)cnt); cnt == 0 gives NaN (0 / 0).
 *  3. base[i] equal to one of the mask values: out[i] = base[i] bit for bit (a NaN payload too).  mask_values (HOST,
 *     nmask in 0..2): the variable's `_FillValue` and / or `missing_value`, or NetCDF's default fill value when it has
 *     neither - the caller's choice; each is rounded to B and compared with ==, a NaN mask value masks NaN cells.
 *  4. otherwise out[i] = (B)(base[i] + mean), the addition in the promoted type of B and X: float32 + float32 is one
 *     float32 addition, float32 + float64 one float64 addition rounded once, float64 + either a float64 addition.  A NaN
 *     mean gives NaN, as the reference writes it.
 * A grid of one cell (n == 1) is summed in another order, as numpy does it: the records then lie contiguous and numpy's
 * reduction adds them pairwise (fewer than 8 one after the other; up to 128 in eight partial sums r[j] += x'[8 k + j]
 * combined as ((r0 + r1) + (r2 + r3)) + ((r4 + r5) + (r6 + r7)), the n % 8 last ones added to that; more are halved at
 * n2 = n / 2 - (n / 2) % 8); tot = 0.0 + that sum.  From two cells on it is step 1.
 * All four (dtype_base, dtype_x) pairs.  base = out = NULL: the mean alone.  out may be base (in place).  mean (n) of
 * dtype_x, may be NULL: the result of step 2.  n_masked, n_new_nan (HOST, may be NULL): the masked cells, and the
 * unmasked cells whose base was not NaN and whose result is.  The entry synchronises.
 * A lane takes 16 bytes of a record when n and every address allow it (PGW_OPT_FORCE_VEC1: one cell); byte offsets into x
 * are 32-bit while it is smaller than 4 GiB (PGW_OPT_FORCE_OFF64: 64-bit); the same bits in every form.  Not timed by the
 * launch profiler.  PGW_ERR_ARG, and nothing launched, for: an unknown dtype, nrec < 1, n < 1, x == NULL, base without
 * out or out without base, nmask outside 0..2. */
int pgw_time_mean_add(pgw_ctx *ctx, int dtype_base, int dtype_x, int nrec, long long n, const void *base, int nmask,
                      const double *mask_values, const void *x, void *out, void *mean, long long *n_masked,
                      long long *n_new_nan);

/* s5 `cdo sub` of two climatology files                  step_01_extract_deltas/extract_climate_delta.sh:244-249
 * out[i] = (dtype)((double)a[i] - (double)b[i]) on n elements; NaN (missing) in either operand gives NaN. */
int pgw_field_sub(pgw_ctx *ctx, int dtype, long long n, const void *a, const void *b, void *out);

/* s6 level list, lon-lat box and model-top merge          step_01_extract_deltas/extract_climate_delta.sh:194-208 and
 * CFday_cut_subdomain.sh:28-30 (`cdo sellonlatbox,$box`), Emon_add_top_from_Amon.sh:45-56 (`cdo sellevel` twice and
 * `cdo -O merge`).  A copy of words:
 *   dst[r, lev_dst0 + k, i, j] = src[r, lev_index[k], lat0 + i, (lon0 + j) % nlon_src]
 * src (nrec, nlev_src, nlat_src, nlon_src), dst (nrec, nlev_dst, nlat_sel, nlon_sel): device arrays of elements of
 * `elem_bytes` = 2, 4 or 8 bytes (NetCDF-3 short, int / float, double), copied as unsigned integers of that size - no
 * arithmetic and no dtype tag, so raw big-endian file bytes go through as well as decoded arrays, and every NaN payload,
 * `_FillValue` and packed value is kept bit for bit.  Only levels lev_dst0 .. lev_dst0 + nlev_sel - 1 of dst are written:
 * two calls with different lev_dst0 into one dst are the merge.  A variable without a level axis passes nlev_src = 1;
 * leading dimensions fold into nrec.
 *  lev_index (nlev_sel, HOST, any order, nlev_sel <= 256; NULL = 0 .. nlev_sel - 1): source level of each output level.
 *  lat0, nlat_sel: the source rows lat0 .. lat0 + nlat_sel - 1.  lon0 in [0, nlon_src), nlon_sel in [1, nlon_src]: the
 *  cyclic run of source columns (lon0 + j) mod nlon_src.  src and dst must not overlap.
 * A lane moves 16, 8, 4 or 2 bytes - the widest word that divides nlon_src, nlon_sel and lon0 in bytes and both addresses
 * (PGW_OPT_FORCE_VEC1: one element); byte offsets are 32-bit when both arrays are below 4 GiB (PGW_OPT_FORCE_OFF64: 64-bit).
 * The same bytes in every form.  Not timed by the launch profiler (pgw_timer_start / _stop around the call do). */
int pgw_select_box(pgw_ctx *ctx, int elem_bytes, int nrec, int nlev_src, int nlat_src, int nlon_src, const void *src,
                   int nlev_sel, const int *lev_index, int lat0, int nlat_sel, int lon0, int nlon_sel, int nlev_dst,
                   int lev_dst0, void *dst);

/* s7 lon-lat box on a curvilinear grid                     step_01_extract_deltas/extract_climate_delta.sh:120-123, 194-208
 * (`cdo sellonlatbox,$box` in front of the Omon / SImon tables, whose files carry 2-D latitude / longitude).  Marks the
 * cells of lat / lon (nj, ni; device arrays of `dtype`) that lie inside box = (lon1, lon2, lat1, lat2) (HOST doubles):
 *   inside[j, i] = lat and lon both finite, min(lat1, lat2) <= lat <= max(lat1, lat2), and lon + 360 k <= lon2 for the
 *   smallest integer k with lon + 360 k >= lon1 (k = ceil((lon1 - lon) / 360), then k += (lon + 360 k < lon1), then
 *   k -= (lon + 360 (k - 1) >= lon1)).  float64 arithmetic, float32 coordinates widened exactly; edges inclusive; NaN and
 *   +-inf coordinates are never inside.
 * Outputs (DEVICE): row_any (nj) and col_any (ni), int, 1 where a cell of that row / column is inside and 0 elsewhere;
 * n_inside, one long long, the number of inside cells.  The entry zeroes all three on the stream before the launch and
 * does not synchronise.  Finding the index window from the flags is the caller's (step_01_extract_deltas.curvilinear_box);
 * the cut itself is pgw_select_box.  Not timed by the launch profiler.
 * PGW_ERR_ARG, and nothing written, for: an unknown dtype, nj < 1, ni < 1, nj * ni >= 2^31, a NULL pointer, a NaN in the
 * box, lon1 >= lon2, lon2 - lon1 > 360. */
int pgw_box_mark_2d(pgw_ctx *ctx, int dtype, int nj, int ni, const void *lat, const void *lon, double lon1, double lon2,
                    double lat1, double lat2, int *row_any, int *col_any, long long *n_inside);

/* Diagnostic: the loads of pgw_clim_accumulate on x (nrec, inner) and nothing else, on the same grid, timed under
 * PGW_K_CLIM_READ - what the card gives this access pattern (tools/clim_time.py); no reference counterpart. */
int pgw_test_read_records(pgw_ctx *ctx, int dtype, int nrec, long long inner, const void *x);

/* c1 hydrostatic check: geopotential on a list of pressure levels.  No reference counterpart as a function: it is
 * integ_geopot (functions.py:128-189) evaluated at p_ref = plev[i] for every i in one walk of each column, on the vertical
 * grid of pgw_set_levels (pa_hl = ak + PS * bk, step_03_apply_to_era.py:64-66), and for two states the loop's
 * phi_ref_error (step_03_apply_to_era.py:289, 298) on every level instead of one.
 *  plev (nplev <= 64, HOST, any order): finite and > 1e-4, the guard value of functions.py:135 (else PGW_ERR_ARG).
 *  FIS, PS_a, PS_b (ntime, ncol) of dtype_2d; T_a, QV_a (ntime, nlev, ncol) of dtype_a; T_b, QV_b of dtype_b.
 *  PS_b = T_b = QV_b = NULL: out = phi_a.  Otherwise out = phi_b - phi_a, and with zg_before != NULL
 *    out = (phi_b - phi_a) - g * zg_delta, zg_delta = the records zg_before / zg_after (ntime, nplev, ncol) of dtype_zg,
 *    in the order of plev, interpolated like load_delta (functions.py:288-292; x_hi == 0: zg_before itself, :282-283).
 *  out (ntime, nplev, ncol) float64, rows in the order of plev.  float64 arithmetic on the stored values whatever the
 *  storage types; the float32 roundings of the reference's dtype flow are not reproduced.
 *  Value at p: k* = half level with the smallest non-negative p_hl - p (ties: lowest index, functions.py:160-163), phi =
 *  phi_hl[k*] - Rd Tv[k* - 1] (ln p - ln p_hl[k*]) (:174-179); p equal to a half-level pressure gives phi_hl[k*] bit for
 *  bit.  NaN where no half level has p_hl >= p (the reference raises there, :162-165) or k* = 0 (:176).
 *  nan_count (nplev, HOST, may be NULL): NaN elements of each output row, over all times and columns.
 *  form (two states): 0 = both states in one walk, 1 = state a's walk, then state b's; the same bits.  One launch in
 *  every form, timed under PGW_K_INTEG_GEOPOT. */
int pgw_geopot_on_plev(pgw_ctx *ctx, int dtype_2d, int dtype_a, int dtype_b, int ntime, int nplev, long long ncol,
                       const double *plev, const void *FIS, const void *PS_a, const void *T_a, const void *QV_a,
                       const void *PS_b, const void *T_b, const void *QV_b, int dtype_zg, const void *zg_before,
                       const void *zg_after, double x_hi, double x_new, double g, int form, double *out,
                       long long *nan_count);

/* c2 per-row statistics of x (nrow, ncol) float64 on the device, NaN skipped - what step_03_apply_to_era.py:308 does for
 * one level (`np.abs(phi_ref_error).max()`, skipna) for the table of the hydrostatic check: count, sum, sum of squares
 * and max |x| of every row into the HOST arrays (nrow).  A row without a finite element gives 0, 0, 0, 0.  Partial sums
 * are combined in an order that depends on the shape alone: two calls give the same bits.  Not timed by the profiler. */
int pgw_level_stats(pgw_ctx *ctx, int nrow, long long ncol, const double *x, long long *count, double *sum, double *sumsq,
                    double *maxabs);

/* c3 delta check: T, RH, U, V of an ERA5-like state on a list of pressure levels, and for two states their change and its
 * distance from the climate deltas.  No reference counterpart as a function.  Vertical grid of pgw_set_levels; per
 * column and state pa[k] = akm[k] + PS * bkm[k], RH[k] = specific_to_relative_humidity(QV[k], pa[k], T[k])
 * (functions.py:107-116) and X(p) = interp_extrap_1d(ln pa, X, ln p, 'nan') (functions.py:511-580) for X in (T, RH, U, V):
 * the first k with ln pa[k] equal to or above ln p; equal gives X[k] bit for bit, k = 0 with "above" and no such k give
 * NaN.  A column with pa[nlev-1] < pa[0] or a NaN PS gives NaN on every level; no status is raised.  float64 arithmetic
 * on the stored values whatever the storage types (the float32 roundings of the reference's dtype flow are not
 * reproduced): the bits of pgw_specific_to_relative_humidity_hybrid + pgw_interp_hybrid_to_plev (F64 -> F64,
 * PGW_EXTRAP_NAN) on widened arrays.
 *  plev (1 <= nplev <= 128 = PGW_MAX_PLEV, HOST, any order, repeats allowed): finite and > 1e-4.
 *  PS_a, PS_b (ntime, ncol) of dtype_2d; T, QV, U, V (ntime, nlev, ncol) of dtype_a / dtype_b.
 *  All five b pointers NULL: out = X_a.  Otherwise out = change = X_b - X_a, and with out_error != NULL
 *    out_error = change - delta where plev < ps_hist, else NaN (at and below ps_hist step_03 applies the surface delta,
 *    so the level's delta is no yardstick there; a NaN ps_hist gives NaN).  delta_X: the records rec_before[i] /
 *    rec_after[i] (ntime, nplev, ncol) of dtype_delta in the order of plev, i = 0..3 for (ta, hur, ua, va); ps_hist: the
 *    records ps_hist_before / ps_hist_after (ntime, ncol) of dtype_delta; each interpolated like load_delta
 *    (functions.py:288-292) with its own x_hi[i], x_new[i] (HOST, i = 4: ps_hist); x_hi[i] == 0: the `before` record itself.
 *  out, out_error (4, ntime, nplev, ncol) float64, variables in the order (ta, hur, ua, va), rows in the order of plev.
 *  PGW_ERR_ARG before anything is uploaded or launched, outputs untouched: nplev outside [1, 128], a level not finite or
 *  not > 1e-4, a bad dtype tag, a null required pointer, some but not all b pointers, out_error without two states or
 *  without all ten record pointers, a pointer not aligned to its element.
 *  One launch, timed under PGW_K_HYBRID_TO_PLEV; byte offsets are 32-bit while every array is below 4 GiB
 *  (PGW_OPT_FORCE_OFF64: 64-bit), the same bits. */
int pgw_state_on_plev(pgw_ctx *ctx, int dtype_2d, int dtype_a, int dtype_b, int ntime, int nplev, long long ncol,
                      const double *plev, const void *PS_a, const void *T_a, const void *QV_a, const void *U_a,
                      const void *V_a, const void *PS_b, const void *T_b, const void *QV_b, const void *U_b,
                      const void *V_b, int dtype_delta, const void *const *rec_before, const void *const *rec_after,
                      const void *ps_hist_before, const void *ps_hist_after, const double *x_hi, const double *x_new,
                      double *out, double *out_error);

#ifdef __cplusplus
}
#endif
#endif /* PGW_HIP_H */
