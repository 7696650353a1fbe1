"""Run-time settings with the names the reference's settings.py exports (settings.py:15-150).

Same module-global style as the reference (scripts import the names), same defaults, so a
user's edited settings.py carries over value by value.
"""
i_debug = 2                                            # settings.py:15

file_name_bases = {'SCEN-HIST': '{}_delta.nc', 'HIST': '{}_historical.nc'}   # :20-23
era5_file_name_base = 'cas{:%Y%m%d%H}0000.nc'          # :26

# dimension names, ERA5 file (:30-35), GCM delta files (:38-42), GCM ocean grid (:45-47)
TIME_ERA, LON_ERA, LAT_ERA, LEV_ERA, HLEV_ERA, SOIL_HLEV_ERA = 'time', 'lon', 'lat', 'level', 'level1', 'soil1'
TIME_GCM, LON_GCM, LAT_GCM, PLEV_GCM, LEV_GCM = 'time', 'lon', 'lat', 'plev', 'lev'
TIME_GCM_OCEAN, LON_GCM_OCEAN, LAT_GCM_OCEAN = 'time', 'longitude', 'latitude'

# CMOR name -> variable name in the ERA5 files (:57-104)
var_name_map = dict(
    ta='T', ua='U', va='V', hur='RELHUM', zg='PHI',
    tas=None, hurs=None, tos=None,
    ps='PS', hus='QV', zgs='FIS', ts='T_SKIN', st='T_SO', sftlf='FR_LAND', sic='FR_SEA_ICE',
)

# step_02 regridding (:120-129).  0: separable bilinear regridding, for deltas on a regular lat/lon grid (1-D coordinates).
# 1: the reference's xESMF branch (functions.py:797-810), built natively - bilinear on the sphere from a source grid with
# 2-D coordinates (rotated-pole regional models, curvilinear grids; 1-D coordinates work too) - use it whenever the GCM / RCM
# deltas are not on a regular lat/lon grid.  Neither xESMF nor ESMF is needed.
i_use_xesmf_regridding = 0
# not in the reference: a target point that lies in no source cell gets 0.0 with xESMF 0.6.2 (environment.yml:177), which is
# the default here; True makes it NaN instead
xesmf_unmapped_to_nan = False
nan_interp_kernel_radius = 1000000
nan_interp_sharpness = 4

# surface-pressure adjustment (:140-150)
p_ref_inp = 30000
adj_factor = 0.95
thresh_phi_ref_max_error = 0.15
max_n_iter = 20
i_reinterp = 0

# ---- not in the reference: arithmetic on float32 ERA5 files ----------------------------------
# 'reference': what the reference computes on float32 files - numpy's promotion puts float32 roundings into it
#     (phi_hl stored in FIS' dtype, functions.py:141,149; float32 tav / e_sat of the ERA state; float32 delta_ps and
#     ps_pgw, step_03:182-193) and writes T, QV, U, V as float64 (`era + delta`, step_03:170-173).  The kernels
#     reproduce those roundings (pgw_file_args.ref_dtype = 1), so iteration count and PS follow the reference.
# 'fast': float64 arithmetic on the stored float32 values, float32 outputs (half the output bytes); PS then differs from
#     the reference by a few 1e-7 relative and, when the last pass ends within ~0.03 m2/s2 of the threshold, by one pass.
f32_file_mode = 'reference'

# ---- not in the reference: dtype flow of the function-level API, pgw4era5_amd/functions.py ----------
# 'common': one dtype for all operands of a call - float64 as soon as one of them is - every operand cast to it on the host,
#     float64 arithmetic on the device, the result in that dtype.  What the functions have always done: existing callers keep
#     their bits.
# 'reference': what the reference's functions compute when operands differ in dtype, as they do on float32 ERA5 files (a
#     float32 T beside float64 pressures).  No cast: every operand goes to the device in its own dtype (half the upload for
#     the float32 ones; DeviceArrays of different dtypes are accepted), the kernels follow numpy's promotion operation by
#     operation (phi_hl in the dtype of zgs, functions.py:141,149; float32 tav / e_sat chain, :144, :74-105; float32 value
#     differences in the interpolations, :575-578) and the result has the dtype the reference returns.  This is what an
#     import swap of the reference's own step_03_apply_to_era.py wants on float32 files (INTEGRATION.md route A).  A float32
#     pressure field (float32 ak / bk; no published file) raises NotImplementedError.
# Read at every call; any other value: ValueError.
function_dtype_flow = 'common'

# Output dtype of T, QV, U, V on float32 files in 'reference' mode.  'float64': what the reference writes (`era + delta`
# promotes; the output file is twice the input).  'float32': the same float64 fields, narrowed on the GPU on the way out -
# half the download and half the file written (file I/O is what bounds the end-to-end rate); PS and the pass count are the
# reference's either way.
f32_out_dtype = 'float64'

# ---- not in the reference: the grid of the climate deltas step_03 reads (`-d`) ----------------------------------------------
# 'era5': the files `step_02 regridding` wrote, on the grid of the ERA5 files (the reference's chain).
# 'source': the files `step_02 regridding` would take as `-i` - the smoothed deltas on the GCM's regular lat / lon grid (1-D
#     lat / lon), same file names - regridded on the GPU as they are needed: the surface deltas whole at load, by the calls
#     step_02 makes; a record of ta, hur, ua, va, zg when the instant moves past one (pgw_regrid_plan_apply into the record
#     window of the DeltaSet).  No intermediate files; every output byte is that of the two-step run.  Not with --bands, not
#     with i_use_xesmf_regridding = 1, ERA5 files with 1-D lat / lon axes only.
# 'source_points': the same files, for ERA5 files of any layout - 2-D lat / lon over (rlat, rlon) of a rotated-pole file, a cell
#     list, a mesh: every column of the file is a target of its own at its own (lat, lon) (pgw_points_plan_apply into the record
#     window).  On a mesh file the output bytes are those of 'source'.  Not with --bands, not with i_use_xesmf_regridding = 1.
# `--delta_grid` on the step_03 command line (or PGW_DELTA_GRID) overrides; any other value: ValueError.
delta_grid = 'era5'

# With delta_grid = 'source_points' on a rotated-pole file: None - the ua / va deltas stay eastward / northward -, 'auto' or
# 'POLE_LAT,POLE_LON' - they are turned onto the file's grid-relative directions as they are regridded (one
# pgw_points_plan_apply_wind launch per record of the pair), the bits `step_02 regridding --rotate_winds` writes; same syntax,
# same rule for the pole.  `--rotate_winds` on the step_03 command line (or PGW_ROTATE_WINDS) overrides.  With any other
# delta_grid, or on a mesh file: ValueError.
rotate_winds = None

# The host side of a file call.  True: process_file_device keeps, per context, a plan of everything that stays the same from file
# to file (pointers, shapes, tables, loop controls) and the library brackets the delta records for the instant itself
# (pgw_step03_file_at): one C call per file.  False: the argument struct is put together in Python for every file, as it is
# anyway whenever the plan does not cover the call (delta records not all resident, a member of the ta group on another time
# axis, keep_hur, an instant with a sub-second part).  `PGW_FILE_PLAN=0` / `=1` overrides.  No influence on any result.
file_plan = True

# The end of a file in the library (include/pgw_hip.h PGW_OPT_FINISH_IN_PASS, context option 'finish_in_pass', default on): the
# loop's storing pass writes the final QV of all hybrid levels and PS, and the surface riders run behind the loop launch.
# `PGW_FINISH_IN_PASS=0` gives the riders first and the finalize kernel.  No influence on any result.

# Placement of the level arrays (T, QV, U, V in and out, the vapour-pressure workspace) in the card's memory.  'spread': the
# context draws them so that half lie in one stretch of physical memory and half in another (device.SpreadPool; the quad
# kernel runs 12 % faster than with all of them in one stretch, which is what consecutive hipMallocs give; DESIGN.md section
# 4).  'plain': plain allocations.  `PGW_PLACEMENT` overrides.  No influence on any result.
placement = 'spread'
