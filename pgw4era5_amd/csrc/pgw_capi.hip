// pgw_capi.hip -- C-ABI (include/pgw_hip.h) over the gfx950 kernels in pgw_kernels.h.
// Built as libpgw_hip.so with hipcc --offload-arch=gfx950 (pgw4era5_amd/csrc/Makefile).
#include "../../include/pgw_hip.h"
#include "pgw_kernels.h"
#include "pgw_loop_control.h"

#include <math.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <functional>
#include <string>
#include <type_traits>
#include <vector>

using namespace pgw;

static_assert(LOOP_MAX_PASS == MULTI_MAX_PASS, "pgw_loop_control.h plans launches of up to MULTI_MAX_PASS passes");

struct ProfRec { int kid; hipEvent_t e0, e1; };

struct pgw_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    std::string err;
    long long err_col = -1;
    DevStatus *d_status = nullptr;     // device; [1] = alternate block of the loop passes (cleared by the pass before);
                                       // [2 .. 2 + MULTI_MAX_PASS) = per-pass blocks of the multi-pass loop kernel
    DevStatus *h_status = nullptr;     // pinned host mirror ([0]) + [1 .. 1 + MULTI_MAX_PASS]: read-back of the multi-pass launch,
                                       // [2 + MULTI_MAX_PASS ...): cleared template for the per-pass blocks
    int last_passes_launched = 0;
    pgw_reduce_max_fn reduce_fn = nullptr;      // latitude-band sharding of one file: MAX over the ranks (pgw_set_reduce_hook)
    void *reduce_user = nullptr;
    // protocol state of the band reduces of the file in progress (pgw_step03_file): how many have been made, how long the
    // next one is (passes of the next loop launch), and whether the error being returned is one every band has seen
    int band_reduces = 0, band_next_np = 0;
    bool band_agreed = false;
    // options (pgw_set_option; defaults from the environment, read ONCE in pgw_ctx_create)
    int opt[PGW_OPT_COUNT];
    // vertical grid
    int nlev = 0;
    double *d_levels = nullptr;        // ak | bk | akm | bkm
    std::vector<double> h_akm, h_bkm;
    double h_akN = 0.0, h_bkN = 0.0;   // ak[nlev], bk[nlev] (surface half level)
    double ps_mono_min = 0.0;
    int n_pure = 0;                    // leading full levels with bkm == 0 (pure-pressure levels)
    // plev table cache for vert_interp_delta
    // (the narrow table for an axis of up to MAX_PLEV levels, else the wide one: with_plev)
    std::vector<double> plev_key;
    PlevTable plev_tab;
    PlevTableWide plev_tab_wide;
    double *d_small = nullptr;         // small scratch (tables), 64 KiB
    // named workspaces grown on demand
    // (0 .. 7 may be adopted from the host layer, pgw_ws_adopt; 8: keys, order and histogram of pgw_gauss_interp_points)
    void *ws[9] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    size_t ws_bytes[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    // profiler
    bool prof_on = false;
    std::vector<ProfRec> prof_pending;
    std::vector<hipEvent_t> event_pool;      // recycled profiling events (create/destroy per launch is slow)
    long long prof_count[PGW_K_COUNT];
    double prof_ms[PGW_K_COUNT];
    hipEvent_t t0 = nullptr, t1 = nullptr;
    hipEvent_t status_read = nullptr;  // behind the status read-back of a multi-pass loop launch (no timing)
    unsigned long long last_levels_touched = 0;
    // PGW_OPT_QV_FROM_PASS: did the last file's finalize kernel use the marks of the converged pass, and how many
    // level-columns of QV did that leave it to skip
    bool last_qv_from_pass = false;
    unsigned long long last_qv_skipped = 0;
};

static const size_t SMALL_BYTES = 64 * 1024;
// room behind the status blocks (device and pinned host) for the FusedFirst argument block of k_delta_quad
static const int FUSED_BLOCKS = (int)((sizeof(FusedFirst<double>) + sizeof(DevStatus) - 1) / sizeof(DevStatus));

static int fail(pgw_ctx *ctx, int code, const char *fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    if (ctx) ctx->err = buf;
    return code;
}

#define HIPCHK(ctx, call)                                                                          \
    do {                                                                                           \
        hipError_t e_ = (call);                                                                    \
        if (e_ != hipSuccess)                                                                      \
            return fail(ctx, PGW_ERR_HIP, "%s failed: %s (%s:%d)", #call, hipGetErrorString(e_),   \
                        __FILE__, __LINE__);                                                       \
    } while (0)

// NEED_AS: in a helper that checks for several entries, under the name of the entry that called it
#define NEED_AS(ctx, caller, cond, msg)                                                            \
    do {                                                                                           \
        if (!(cond)) return fail(ctx, PGW_ERR_ARG, "%s: %s", caller, msg);                         \
    } while (0)
#define NEED(ctx, cond, msg) NEED_AS(ctx, __func__, cond, msg)

static const char *status_text(int code) {
    switch (code) {
        case PGW_ERR_SRC_NOT_ASCENDING: return "Source pressure values must be ascending!";
        case PGW_ERR_TARG_NOT_ASCENDING: return "Target pressure values must be ascending!";
        case PGW_ERR_EXTRAP_OFF: return "Extrapolation deactivated but data out of bounds.";
        case PGW_ERR_PREF_BELOW_SURFACE:
            return "p_ref locally lies below the surface. Please set a lower reference pressue (p_ref_inp) in settings.py";
        case PGW_ERR_PREF_AT_TOP: return "p_ref is matched by the top half level (level 0 does not exist)";
        case PGW_ERR_PS_HIST_ABOVE_TOP: return "historical surface pressure is not below the top climate-delta pressure level";
        case PGW_ERR_TOP_PRESSURE:
            return "ERA5 top pressure is lower than climate delta top pressure. If you are certain that you do not need "
                   "the data beyond to upper-most pressure level of the climate delta, you can set the flag "
                   "--ignore_top_pressure_error and re-run the script.";
        case PGW_ERR_NOT_CONVERGED: return "ERROR! Pressure adjustment did not converge";
        case PGW_ERR_GRID_EXTENT:      // functions.py:845-856 / 877-888 ("North or South" / "East or West" is chosen by the host)
            return "ERA5 dataset extends further than GCM dataset!. Perhaps consider using ERA5 on a subdomain only if "
                   "global coverage is not required?";
        case PGW_ERR_NO_P_REF:
            return "No reference pressure level above the required local minimum pressure level could not be found "
                   "everywhere. This is likely the case because your geopotential data set does not reach up high enough "
                   "(e.g. only to 500 hPa instead of e.g. 300 hPa?)";
        default: return "error";
    }
}

// a status code ends the call: the reference's text for it and the column it was found in (-1: none)
static int fail_status(pgw_ctx *ctx, int code, long long col = -1) {
    ctx->err = status_text(code);
    ctx->err_col = col;
    return code;
}

// ------------------------------------------------------------------ launch helpers
struct Prof {
    pgw_ctx *c; int kid; hipEvent_t e0 = nullptr, e1 = nullptr;
    hipEvent_t take() {
        hipEvent_t e = nullptr;
        if (!c->event_pool.empty()) { e = c->event_pool.back(); c->event_pool.pop_back(); }
        else if (hipEventCreate(&e) != hipSuccess) e = nullptr;      // launch goes unprofiled (see ~Prof)
        return e;
    }
    hipStream_t st;
    Prof(pgw_ctx *c_, int kid_, hipStream_t st_ = nullptr) : c(c_), kid(kid_), st(st_ ? st_ : c_->stream) {
        if (c->prof_on) {
            e0 = take(); e1 = take();
            if (e0 && e1) hipEventRecord(e0, st);
            else { if (e0) c->event_pool.push_back(e0); if (e1) c->event_pool.push_back(e1); e0 = e1 = nullptr; }
        }
    }
    ~Prof() {
        if (e0 && e1) {
            hipEventRecord(e1, st);
            c->prof_pending.push_back({kid, e0, e1});
        }
    }
};

static int prof_resolve(pgw_ctx *ctx) {
    if (ctx->prof_pending.empty()) return PGW_OK;
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    for (auto &r : ctx->prof_pending) {
        float ms = 0.f;
        hipEventElapsedTime(&ms, r.e0, r.e1);
        ctx->prof_count[r.kid] += 1;
        ctx->prof_ms[r.kid] += ms;
        ctx->event_pool.push_back(r.e0); ctx->event_pool.push_back(r.e1);
    }
    ctx->prof_pending.clear();
    return PGW_OK;
}

static inline unsigned int nblocks(long long n, int per) { return (unsigned int)((n + per - 1) / per); }

static inline bool aligned16(const void *p) { return p == nullptr || (((uintptr_t)p) & 15) == 0; }

// columns per thread: 16 B per lane when shape and alignment allow, else 1
// `max_v` caps the width for kernels whose register footprint makes the widest form slower.
// the widest form `v` the options, the alignment of every operand and the row length allow
static int fit_vec(pgw_ctx *ctx, int v, long long ncol, std::initializer_list<const void *> ptrs) {
    if (ctx->opt[PGW_OPT_FORCE_VEC1]) return 1;          // test knob: scalar columns per thread
    for (const void *p : ptrs) if (!aligned16(p)) return 1;
    while (v > 1 && ncol % v != 0) v >>= 1;
    return v;
}
static int pick_vec(pgw_ctx *ctx, int dtype, long long ncol, std::initializer_list<const void *> ptrs, int max_v = 4) {
    int v = (dtype == PGW_F64) ? 2 : 4;
    if (v > max_v) v = max_v;
    return fit_vec(ctx, v, ncol, ptrs);
}

static inline size_t elem_size(int dtype) { return dtype == PGW_F64 ? 8 : 4; }

// blocks of a grid-stride kernel over n items: at most 16 for each of 256 CUs
static inline unsigned int flat_grid(long long n) {
    const unsigned int nb = nblocks(n, BLOCK), cap = 256 * 16;
    return nb > cap ? cap : nb;
}

// a status block no kernel has reported into
static DevStatus blank_status() {
    DevStatus z;
    memset(&z, 0, sizeof(z));
    z.col = z.min_targ_bits = z.min_src_bits = ~0ull;
    return z;
}

static int status_reset(pgw_ctx *ctx) {
    *ctx->h_status = blank_status();
    HIPCHK(ctx, hipMemcpyAsync(ctx->d_status, ctx->h_status, sizeof(DevStatus), hipMemcpyHostToDevice, ctx->stream));
    return PGW_OK;
}
static int status_fetch(pgw_ctx *ctx, const DevStatus *from = nullptr) {
    HIPCHK(ctx, hipMemcpyAsync(ctx->h_status, from ? from : ctx->d_status, sizeof(DevStatus), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return PGW_OK;
}
static int status_check(pgw_ctx *ctx, const DevStatus *from = nullptr) {
    int rc = status_fetch(ctx, from);
    if (rc) return rc;
    if (ctx->h_status->code != 0) {
        int code;
        ordered_status(*ctx->h_status, &code, &ctx->err_col);
        return fail_status(ctx, code, ctx->err_col);
    }
    return PGW_OK;
}

static int ws_get(pgw_ctx *ctx, int slot, size_t bytes, void **out) {
    if (ctx->ws_bytes[slot] < bytes) {
        if (ctx->ws[slot]) { HIPCHK(ctx, hipStreamSynchronize(ctx->stream)); HIPCHK(ctx, hipFree(ctx->ws[slot])); }
        ctx->ws[slot] = nullptr; ctx->ws_bytes[slot] = 0;
        HIPCHK(ctx, hipMalloc(&ctx->ws[slot], bytes));
        ctx->ws_bytes[slot] = bytes;
    }
    *out = ctx->ws[slot];
    return PGW_OK;
}

static Levels levels_of(pgw_ctx *ctx) {
    Levels lv;
    int n = ctx->nlev;
    lv.ak = ctx->d_levels;
    lv.bk = ctx->d_levels + (n + 1);
    lv.akm = ctx->d_levels + 2 * (n + 1);
    lv.bkm = ctx->d_levels + 2 * (n + 1) + n;
    lv.nlev = n;
    lv.ps_mono_min = ctx->ps_mono_min;
    return lv;
}

// ------------------------------------------------------------------ context
extern "C" const char *pgw_version(void) { return "pgw_hip 0.1.0 (gfx950)"; }

extern "C" int pgw_device_count(int *n) {
    int c = 0;
    hipError_t e = hipGetDeviceCount(&c);
    if (e != hipSuccess) { *n = 0; return PGW_ERR_HIP; }
    *n = c;
    return PGW_OK;
}

extern "C" int pgw_device_pci_bus_id(int device, char *buf, int len) {
    if (!buf || len < 13) return PGW_ERR_ARG;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || device < 0 || device >= n) { (void)hipGetLastError(); buf[0] = 0; return PGW_ERR_ARG; }
    hipError_t e = hipDeviceGetPCIBusId(buf, len, device);
    if (e != hipSuccess) { (void)hipGetLastError(); buf[0] = 0; return PGW_ERR_HIP; }   // not left behind for a later hipGetLastError()
    return PGW_OK;
}

static int env_flag(const char *name, int dflt) {
    const char *e = getenv(name);
    if (!e || !e[0]) return dflt;
    return (e[0] == '0') ? 0 : 1;
}

extern "C" int pgw_ctx_create(int device, pgw_ctx **out) {
    if (!out) return PGW_ERR_ARG;
    *out = nullptr;
    int cnt = 0;
    if (hipGetDeviceCount(&cnt) != hipSuccess || cnt <= 0) return PGW_ERR_HIP;
    if (device < 0 || device >= cnt) return PGW_ERR_ARG;
    if (hipSetDevice(device) != hipSuccess) return PGW_ERR_HIP;
    pgw_ctx *c = new pgw_ctx();
    c->device = device;
    memset(c->prof_count, 0, sizeof(c->prof_count));
    memset(c->prof_ms, 0, sizeof(c->prof_ms));
    // the environment is read here and nowhere else (no getenv on the launch path)
    c->opt[PGW_OPT_QUAD] = env_flag("PGW_QUAD", 1);
    c->opt[PGW_OPT_FULL_COLUMN] = env_flag("PGW_FULL_COLUMN", 0);
    c->opt[PGW_OPT_FORCE_VEC1] = env_flag("PGW_FORCE_VEC1", 0);
    c->opt[PGW_OPT_MULTIPASS] = env_flag("PGW_MULTIPASS", 1);
    c->opt[PGW_OPT_LOOP_GUESS] = 6;
    c->opt[PGW_OPT_FORCE_OFF64] = 0;
    c->opt[PGW_OPT_TEST_FAIL] = 0;
    c->opt[PGW_OPT_FUSED_FIRST] = env_flag("PGW_FUSED_FIRST", 1);
    c->opt[PGW_OPT_QV_FROM_PASS] = env_flag("PGW_QV_FROM_PASS", 1);
    c->opt[PGW_OPT_FINISH_IN_PASS] = env_flag("PGW_FINISH_IN_PASS", 1);
    c->opt[PGW_OPT_MIXED_VEC] = 4;
    c->opt[PGW_OPT_SPARSE_DIRECT] = 0;
    if (hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess ||
        hipMalloc(&c->d_status, (2 + MULTI_MAX_PASS + FUSED_BLOCKS) * sizeof(DevStatus)) != hipSuccess ||
        hipHostMalloc(&c->h_status, (2 + 2 * MULTI_MAX_PASS + FUSED_BLOCKS) * sizeof(DevStatus)) != hipSuccess ||
        hipMalloc(&c->d_small, SMALL_BYTES) != hipSuccess ||
        hipEventCreate(&c->t0) != hipSuccess || hipEventCreate(&c->t1) != hipSuccess ||
        hipEventCreateWithFlags(&c->status_read, hipEventDisableTiming) != hipSuccess) {
        pgw_ctx_destroy(c);            // releases whatever was created before the failure
        return PGW_ERR_HIP;
    }
    *out = c;
    return PGW_OK;
}

extern "C" int pgw_ctx_destroy(pgw_ctx *ctx) {
    if (!ctx) return PGW_OK;
    hipSetDevice(ctx->device);
    if (ctx->stream) hipStreamSynchronize(ctx->stream);
    for (auto &r : ctx->prof_pending) { hipEventDestroy(r.e0); hipEventDestroy(r.e1); }
    for (auto &e : ctx->event_pool) hipEventDestroy(e);
    for (int i = 0; i < 9; ++i) if (ctx->ws[i]) hipFree(ctx->ws[i]);
    if (ctx->d_levels) hipFree(ctx->d_levels);
    if (ctx->d_small) hipFree(ctx->d_small);
    if (ctx->d_status) hipFree(ctx->d_status);
    if (ctx->h_status) hipHostFree(ctx->h_status);
    if (ctx->t0) hipEventDestroy(ctx->t0);
    if (ctx->t1) hipEventDestroy(ctx->t1);
    if (ctx->status_read) hipEventDestroy(ctx->status_read);
    if (ctx->stream) hipStreamDestroy(ctx->stream);
    delete ctx;
    return PGW_OK;
}

extern "C" int pgw_set_option(pgw_ctx *ctx, int option, int value) {
    if (!ctx) return PGW_ERR_ARG;
    if (option < 0 || option >= PGW_OPT_COUNT) return fail(ctx, PGW_ERR_ARG, "pgw_set_option: unknown option %d", option);
    ctx->opt[option] = value;
    return PGW_OK;
}
extern "C" int pgw_get_option(pgw_ctx *ctx, int option, int *value) {
    if (!ctx || !value) return PGW_ERR_ARG;
    if (option < 0 || option >= PGW_OPT_COUNT) return fail(ctx, PGW_ERR_ARG, "pgw_get_option: unknown option %d", option);
    *value = ctx->opt[option];
    return PGW_OK;
}

extern "C" const char *pgw_last_error(pgw_ctx *ctx) { return ctx ? ctx->err.c_str() : "no context"; }
extern "C" long long pgw_error_column(pgw_ctx *ctx) { return ctx ? ctx->err_col : -1; }

extern "C" int pgw_device_name(pgw_ctx *ctx, char *buf, size_t len) {
    hipDeviceProp_t p;
    HIPCHK(ctx, hipGetDeviceProperties(&p, ctx->device));
    snprintf(buf, len, "%s (%s, %d CUs)", p.name, p.gcnArchName, p.multiProcessorCount);
    return PGW_OK;
}

// ------------------------------------------------------------------ memory
extern "C" int pgw_malloc(pgw_ctx *ctx, size_t bytes, void **dptr) {
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const hipError_t e = hipMalloc(dptr, bytes ? bytes : 16);
    if (e != hipSuccess) {
        // an allocation that does not fit is an answer, not a fault of the context: clear HIP's sticky last error so that the
        // hipGetLastError() after the next kernel launch does not report it (the placement draw probes how much fits)
        (void)hipGetLastError();
        *dptr = nullptr;
        return fail(ctx, PGW_ERR_HIP, "hipMalloc(%zu bytes) failed: %s", bytes, hipGetErrorString(e));
    }
    return PGW_OK;
}
extern "C" int pgw_free(pgw_ctx *ctx, void *dptr) {
    if (!dptr) return PGW_OK;
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    HIPCHK(ctx, hipFree(dptr));
    return PGW_OK;
}
extern "C" int pgw_host_alloc(pgw_ctx *ctx, size_t bytes, void **hptr) {
    HIPCHK(ctx, hipSetDevice(ctx->device));                  // callable from reader / writer threads
    HIPCHK(ctx, hipHostMalloc(hptr, bytes ? bytes : 16));
    return PGW_OK;
}
extern "C" int pgw_host_free(pgw_ctx *ctx, void *hptr) {
    if (hptr) HIPCHK(ctx, hipHostFree(hptr));
    return PGW_OK;
}
extern "C" int pgw_memcpy_h2d(pgw_ctx *ctx, void *dst, const void *src, size_t bytes) {
    if (bytes) HIPCHK(ctx, hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, ctx->stream));
    return PGW_OK;
}
extern "C" int pgw_memcpy_d2h(pgw_ctx *ctx, void *dst, const void *src, size_t bytes) {
    if (bytes) HIPCHK(ctx, hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, ctx->stream));
    return PGW_OK;
}
extern "C" int pgw_memcpy_d2d(pgw_ctx *ctx, void *dst, const void *src, size_t bytes) {
    if (bytes) HIPCHK(ctx, hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, ctx->stream));
    return PGW_OK;
}
extern "C" int pgw_memset(pgw_ctx *ctx, void *dst, int value, size_t bytes) {
    if (bytes) HIPCHK(ctx, hipMemsetAsync(dst, value, bytes, ctx->stream));
    return PGW_OK;
}
extern "C" int pgw_sync(pgw_ctx *ctx) {
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return PGW_OK;
}
extern "C" int pgw_mem_info(pgw_ctx *ctx, size_t *free_bytes, size_t *total_bytes) {
    HIPCHK(ctx, hipSetDevice(ctx->device));
    HIPCHK(ctx, hipMemGetInfo(free_bytes, total_bytes));
    return PGW_OK;
}

// ------------------------------------------------------------------ profiler / timer
extern "C" int pgw_profile_enable(pgw_ctx *ctx, int on) {
    int rc = prof_resolve(ctx);
    ctx->prof_on = on != 0;
    return rc;
}
extern "C" int pgw_profile_reset(pgw_ctx *ctx) {
    int rc = prof_resolve(ctx);
    memset(ctx->prof_count, 0, sizeof(ctx->prof_count));
    memset(ctx->prof_ms, 0, sizeof(ctx->prof_ms));
    return rc;
}
extern "C" int pgw_profile_get(pgw_ctx *ctx, int kid, long long *launches, double *total_ms) {
    NEED(ctx, kid >= 0 && kid < PGW_K_COUNT, "bad kernel id");
    int rc = prof_resolve(ctx);
    if (launches) *launches = ctx->prof_count[kid];
    if (total_ms) *total_ms = ctx->prof_ms[kid];
    return rc;
}
extern "C" int pgw_timer_start(pgw_ctx *ctx) {
    HIPCHK(ctx, hipEventRecord(ctx->t0, ctx->stream));
    return PGW_OK;
}
extern "C" int pgw_timer_stop(pgw_ctx *ctx, double *ms) {
    HIPCHK(ctx, hipEventRecord(ctx->t1, ctx->stream));
    HIPCHK(ctx, hipEventSynchronize(ctx->t1));
    float f = 0.f;
    HIPCHK(ctx, hipEventElapsedTime(&f, ctx->t0, ctx->t1));
    if (ms) *ms = f;
    return PGW_OK;
}

// ------------------------------------------------------------------ vertical grid
extern "C" int pgw_set_levels(pgw_ctx *ctx, int nlev, const double *ak, const double *bk,
                              const double *akm, const double *bkm) {
    NEED(ctx, nlev >= 1 && nlev <= MAX_NLEV && ak && bk, "nlev must be in [1, 256]");
    NEED(ctx, (akm == nullptr) == (bkm == nullptr), "akm and bkm must both be given or both be NULL");
    std::vector<double> h((size_t)4 * nlev + 2);
    double *pak = h.data(), *pbk = pak + nlev + 1, *pakm = pbk + nlev + 1, *pbkm = pakm + nlev;
    memcpy(pak, ak, sizeof(double) * (nlev + 1));
    memcpy(pbk, bk, sizeof(double) * (nlev + 1));
    for (int l = 0; l < nlev; ++l) {
        if (akm) { pakm[l] = akm[l]; pbkm[l] = bkm[l]; }
        else {   // step_03_apply_to_era.py:74-85: 0.5*diff(label='lower') + lower
            pakm[l] = 0.5 * (ak[l + 1] - ak[l]) + ak[l];
            pbkm[l] = 0.5 * (bk[l + 1] - bk[l]) + bk[l];
        }
    }
    // smallest ps for which ak + ps*bk is strictly ascending over all layers:
    // d(ak) + ps*d(bk) > 0.  Layers with d(bk) <= 0 need d(ak) + ps*d(bk) > 0 for all ps of
    // interest; if d(bk) < 0 or (d(bk) == 0 and d(ak) <= 0) monotonicity is never assumed.
    double pmin = 0.0;
    for (int l = 0; l < nlev; ++l) {
        double da = ak[l + 1] - ak[l], db = bk[l + 1] - bk[l];
        if (db > 0) { double need = -da / db; if (need >= pmin) pmin = nextafter(need, INFINITY); }
        else if (db == 0 && da > 0) { /* fine for every ps */ }
        else { pmin = INFINITY; break; }
    }
    if (ctx->nlev != nlev || !ctx->d_levels) {
        if (ctx->d_levels) { HIPCHK(ctx, hipStreamSynchronize(ctx->stream)); HIPCHK(ctx, hipFree(ctx->d_levels)); ctx->d_levels = nullptr; }
        HIPCHK(ctx, hipMalloc(&ctx->d_levels, sizeof(double) * h.size()));
    }
    HIPCHK(ctx, hipMemcpyAsync(ctx->d_levels, h.data(), sizeof(double) * h.size(), hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));     // h is a stack-lifetime buffer
    ctx->nlev = nlev;
    ctx->h_akN = ak[nlev]; ctx->h_bkN = bk[nlev];
    ctx->ps_mono_min = pmin;
    ctx->n_pure = 0;
    while (ctx->n_pure < nlev && pbkm[ctx->n_pure] == 0.0) ctx->n_pure += 1;
    ctx->h_akm.assign(pakm, pakm + nlev);
    ctx->h_bkm.assign(pbkm, pbkm + nlev);
    return PGW_OK;
}

extern "C" int pgw_get_full_level_coeffs(pgw_ctx *ctx, double *akm_out, double *bkm_out) {
    NEED(ctx, ctx->nlev > 0, "pgw_set_levels has not been called");
    memcpy(akm_out, ctx->h_akm.data(), sizeof(double) * ctx->nlev);
    memcpy(bkm_out, ctx->h_bkm.data(), sizeof(double) * ctx->nlev);
    return PGW_OK;
}

// every compute entry binds the context's device first: a process may hold contexts on several devices
#define CHECK_COMMON(ctx, dtype, ntime, ncol)                                        \
    NEED(ctx, dtype == PGW_F32 || dtype == PGW_F64, "dtype must be PGW_F32 or PGW_F64"); \
    NEED(ctx, ntime >= 1 && ncol >= 1, "ntime and ncol must be positive");           \
    HIPCHK(ctx, hipSetDevice(ctx->device));

// ------------------------------------------------------------------ dispatch
// A run-time tag becomes the type of an argument of the generic lambda `f`: f(T()) for a storage type,
// f(std::integral_constant<int, V>()) for a constant.  What a dispatcher does not call is not instantiated.
template <int N> using int_c = std::integral_constant<int, N>;
#define TAG_OK(t) ((t) == PGW_F32 || (t) == PGW_F64)
template <typename F> static inline void with_type(int tag, F &&f) { if (tag == PGW_F64) f(double()); else f(float()); }
template <typename F> static inline void with_vec(int vec, F &&f) {
    if (vec == 4) f(int_c<4>());
    else if (vec == 2) f(int_c<2>());
    else f(int_c<1>());
}
// storage dtype and vector width: float64 V = 2, 1; float32 V = 4, 2, 1
template <typename F> static inline void with_type_vec(int dtype, int vec, F &&f) {
    if (dtype == PGW_F64) { if (vec == 2) f(double(), int_c<2>()); else f(double(), int_c<1>()); }
    else with_vec(vec, [&](auto v_) { f(float(), v_); });
}
// storage type T of the ERA5 fields, TL of the PGW level arrays (ta_pgw, e, QV out), REF = reference-dtype mode
// (float32 files only: T = float, TL = double): f(T(), TL(), std::bool_constant<REF>())
template <typename F> static inline void with_flow(int dtype, bool ref, F &&f) {
    if (dtype == PGW_F64) f(double(), double(), std::false_type());
    else if (ref) f(float(), double(), std::true_type());
    else f(float(), float(), std::false_type());
}
// ... and vector width: float64 levels V = 2, 1; float32 levels V = 4, 2, 1
template <typename F> static inline void with_flow_vec(int dtype, bool ref, int vec, F &&f) {
    with_flow(dtype, ref, [&](auto t_, auto l_, auto ref_) {
        if constexpr (sizeof(l_) == 8) { if (vec >= 2) f(t_, l_, ref_, int_c<2>()); else f(t_, l_, ref_, int_c<1>()); }
        else with_vec(vec, [&](auto v_) { f(t_, l_, ref_, v_); });
    });
}
// a run-time integer as f(int_c<i>()): `extrapolate`, `which`, a flag; the caller has checked that it lies in [0, N)
template <typename F, int... I> static inline void with_int_(int i, F &&f, std::integer_sequence<int, I...>) { ((i == I ? f(int_c<I>()) : (void)0), ...); }
template <int N, typename F> static inline void with_int(int i, F &&f) { with_int_(i, f, std::make_integer_sequence<int, N>()); }
// 32-bit byte offsets from uniform bases when every array is smaller than 4 GiB
template <typename F> static inline void with_offsets(bool o32, F &&f) { if (o32) f(boff32()); else f(boff64()); }

// Record source bracketing an instant; the record after it is not read when the instant is the record before (x_hi == 0).
template <typename T> static inline DeltaSrc<T> delta_src(const void *before, const void *after, double x_hi, double x_new) {
    return DeltaSrc<T>{(const T *)before, x_hi == 0.0 ? nullptr : (const T *)after, x_hi, x_new};
}
template <typename T> static inline PairSrc<T> pair_src(const void *b0, const void *a0, const void *b1, const void *a1, double x_hi,
                                                        double x_new) {
    return PairSrc<T>{delta_src<T>(b0, a0, x_hi, x_new), delta_src<T>(b1, a1, x_hi, x_new)};
}

// The riders' soil table (step_03:139-140): the layer count checked, w = exp(-depth / 2.8) in float64 on the host.
// `caller` names the entry in the status text.  soil_depth may be NULL where no soil output is asked for (the callers check
// that after the layer count): the weights then stay 0 and no kernel reads them.
static int soil_table(pgw_ctx *ctx, const char *caller, int nsoil, const double *soil_depth, SoilTable *st) {
    NEED_AS(ctx, caller, nsoil >= 0 && nsoil <= MAX_SOIL, "nsoil must be in [0, 16]");
    memset(st, 0, sizeof(*st));
    st->n = nsoil;
    for (int s = 0; soil_depth && s < nsoil; ++s) st->w[s] = exp(-soil_depth[s] / 2.8);      // step_03:140
    return PGW_OK;
}

extern "C" int pgw_pressure_levels(pgw_ctx *ctx, int dtype, int ntime, long long ncol,
                                   const void *ps, void *pa_hl, void *pa) {
    CHECK_COMMON(ctx, dtype, ntime, ncol);
    NEED(ctx, ctx->nlev > 0, "pgw_set_levels has not been called");
    NEED(ctx, ps && (pa_hl || pa), "null pointer");
    int vec = pick_vec(ctx, dtype, ncol, {ps, pa_hl, pa});
    Levels lv = levels_of(ctx);
    {
        Prof pr(ctx, PGW_K_PRESSURE);
        with_type_vec(dtype, vec, [&](auto t_, auto v_) {
            using T = decltype(t_);
            constexpr int V = decltype(v_)::value;
            hipLaunchKernelGGL((k_pressure_levels<T, V>), dim3(nblocks((long long)ntime * ncol / V, BLOCK)), dim3(BLOCK), 0,
                               ctx->stream, lv, ntime, ncol, (const T *)ps, (T *)pa_hl, (T *)pa);
        });
    }
    HIPCHK(ctx, hipGetLastError());
    return PGW_OK;
}

// ------------------------------------------------------------------ humidity
template <int MODE>
static int humidity_flat(pgw_ctx *ctx, int kid, int dtype, long long n, const void *x, const void *pa,
                         const void *ta, void *out) {
    NEED(ctx, dtype == PGW_F32 || dtype == PGW_F64, "dtype must be PGW_F32 or PGW_F64");
    NEED(ctx, n >= 1 && x && pa && ta && out, "bad argument");
    int vec = pick_vec(ctx, dtype, n, {x, pa, ta, out});
    const unsigned int nb = flat_grid(n / vec);
    {
        Prof pr(ctx, kid);
        with_type_vec(dtype, vec, [&](auto t_, auto v_) {
            using T = decltype(t_);
            hipLaunchKernelGGL((k_humidity_flat<T, decltype(v_)::value, MODE>), dim3(nb), dim3(BLOCK), 0, ctx->stream, n,
                               (const T *)x, (const T *)pa, (const T *)ta, (T *)out);
        });
    }
    HIPCHK(ctx, hipGetLastError());
    return PGW_OK;
}
extern "C" int pgw_specific_to_relative_humidity(pgw_ctx *ctx, int dtype, long long n, const void *hus,
                                                 const void *pa, const void *ta, void *hur) {
    return humidity_flat<0>(ctx, PGW_K_Q_TO_RH, dtype, n, hus, pa, ta, hur);
}
extern "C" int pgw_relative_to_specific_humidity(pgw_ctx *ctx, int dtype, long long n, const void *hur,
                                                 const void *pa, const void *ta, void *hus) {
    return humidity_flat<1>(ctx, PGW_K_RH_TO_Q, dtype, n, hur, pa, ta, hus);
}

extern "C" int pgw_humidity_leaf(pgw_ctx *ctx, int dtype, int which, long long n, const void *a, const void *b, void *out) {
    NEED(ctx, dtype == PGW_F32 || dtype == PGW_F64, "dtype must be PGW_F32 or PGW_F64");
    NEED(ctx, which >= 0 && which <= 4, "which must be 0..4");
    NEED(ctx, n >= 1 && a && out && (which >= 2 || b), "bad argument");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const unsigned int nb = flat_grid(n);
    with_type(dtype, [&](auto t_) { with_int<5>(which, [&](auto w_) {
        using T = decltype(t_);
        hipLaunchKernelGGL((k_humidity_leaf<T, decltype(w_)::value>), dim3(nb), dim3(BLOCK), 0, ctx->stream, n, (const T *)a,
                           (const T *)b, (T *)out);
    }); });
    HIPCHK(ctx, hipGetLastError());
    return PGW_OK;
}

template <int MODE>
static int humidity_hybrid(pgw_ctx *ctx, int kid, int dtype, int ntime, long long ncol, const void *x,
                           const void *ps, const void *ta, void *out) {
    CHECK_COMMON(ctx, dtype, ntime, ncol);
    NEED(ctx, ctx->nlev > 0, "pgw_set_levels has not been called");
    NEED(ctx, x && ps && ta && out, "null pointer");
    int vec = pick_vec(ctx, dtype, ncol, {x, ps, ta, out});
    Levels lv = levels_of(ctx);
    {
        Prof pr(ctx, kid);
        with_type_vec(dtype, vec, [&](auto t_, auto v_) {
            using T = decltype(t_);
            constexpr int V = decltype(v_)::value;
            hipLaunchKernelGGL((k_humidity_hybrid<T, V, MODE>), dim3(nblocks((long long)ntime * ncol / V, BLOCK)), dim3(BLOCK), 0,
                               ctx->stream, lv, ntime, ncol, (const T *)x, (const T *)ps, (const T *)ta, (T *)out);
        });
    }
    HIPCHK(ctx, hipGetLastError());
    return PGW_OK;
}
extern "C" int pgw_specific_to_relative_humidity_hybrid(pgw_ctx *ctx, int dtype, int ntime, long long ncol,
                                                        const void *hus, const void *ps, const void *ta, void *hur) {
    return humidity_hybrid<0>(ctx, PGW_K_Q_TO_RH, dtype, ntime, ncol, hus, ps, ta, hur);
}
extern "C" int pgw_relative_to_specific_humidity_hybrid(pgw_ctx *ctx, int dtype, int ntime, long long ncol,
                                                        const void *hur, const void *ps, const void *ta, void *hus) {
    return humidity_hybrid<1>(ctx, PGW_K_RH_TO_Q, dtype, ntime, ncol, hur, ps, ta, hus);
}

// ------------------------------------------------------------------ integ_geopot
static int launch_integ_geopot(pgw_ctx *ctx, int dtype, int nlev, int ntime, long long ncol, const void *pa_hl,
                               const void *zgs, const void *ta, const void *hus, double p_ref,
                               const void *p_ref_field, void *phi_ref, int full_column) {
    int vec = pick_vec(ctx, dtype, ncol, {pa_hl, zgs, ta, hus, p_ref_field, phi_ref});
    Prof pr(ctx, PGW_K_INTEG_GEOPOT);
    with_type_vec(dtype, vec, [&](auto t_, auto v_) {
        using T = decltype(t_);
        constexpr int V = decltype(v_)::value;
        // 4 levels per chunk: 2 / 4 / 8 measured the same
        hipLaunchKernelGGL((k_integ_geopot<T, V, 4, T>), dim3(nblocks((long long)ntime * ncol / V, BLOCK)), dim3(BLOCK), 0,
                           ctx->stream, nlev, ntime, ncol, (const T *)pa_hl, (const T *)zgs, (const T *)ta, (const T *)hus, p_ref,
                           (const T *)p_ref_field, (T *)phi_ref, full_column, ctx->d_status);
    });
    return PGW_OK;
}

extern "C" int pgw_integ_geopot(pgw_ctx *ctx, int dtype, int ntime, int nlev, long long ncol, const void *pa_hl,
                                const void *zgs, const void *ta, const void *hus, double p_ref,
                                const void *p_ref_field, void *phi_ref, int full_column) {
    CHECK_COMMON(ctx, dtype, ntime, ncol);
    NEED(ctx, nlev >= 1, "nlev must be positive");
    NEED(ctx, pa_hl && zgs && ta && hus && phi_ref, "null pointer");
    int rc = status_reset(ctx);
    if (rc) return rc;
    launch_integ_geopot(ctx, dtype, nlev, ntime, ncol, pa_hl, zgs, ta, hus, p_ref, p_ref_field, phi_ref, full_column);
    HIPCHK(ctx, hipGetLastError());
    return status_check(ctx);
}

// ------------------------------------------------------------------ interp_logp_4d
extern "C" int pgw_interp_logp_4d(pgw_ctx *ctx, int dtype, int ntime, int nsrc, int ntarg, long long ncol,
                                  const void *var, const void *source_P, const void *targ_P, int extrapolate,
                                  int logp_in, void *out) {
    CHECK_COMMON(ctx, dtype, ntime, ncol);
    NEED(ctx, nsrc >= 2 && ntarg >= 1, "need at least 2 source levels and 1 target level");
    NEED(ctx, var && source_P && targ_P && out, "null pointer");
    if (extrapolate < 0 || extrapolate > 3) return fail(ctx, PGW_ERR_ARG, "Invalid input value for \"extrapolate\"");
    int rc = status_reset(ctx);
    if (rc) return rc;
    {
        Prof pr(ctx, PGW_K_INTERP_LOGP);
        with_type(dtype, [&](auto t_) { with_int<4>(extrapolate, [&](auto m_) {
            using T = decltype(t_);
            hipLaunchKernelGGL((k_interp_logp_stream<T, T, T, decltype(m_)::value>), dim3(nblocks((long long)ntime * ncol, BLOCK)),
                               dim3(BLOCK), 0, ctx->stream, ntime, nsrc, ntarg, ncol, (const T *)var, (const T *)source_P,
                               (const T *)targ_P, (T *)out, logp_in, ctx->d_status);
        }); });
    }
    HIPCHK(ctx, hipGetLastError());
    return status_check(ctx);
}

// ------------------------------------------------------------------ step_01: model levels -> pressure levels
#ifndef PGW_H2P_MAX_V
#define PGW_H2P_MAX_V 1
#endif
constexpr int H2P_MAX_V = PGW_H2P_MAX_V;      // 1 or 2 columns per thread of k_hybrid_to_plev (see pgw_interp_hybrid_to_plev)
static_assert(H2P_MAX_V == 1 || H2P_MAX_V == 2, "PGW_H2P_MAX_V");

extern "C" int pgw_interp_hybrid_to_plev(pgw_ctx *ctx, int dtype_in, int dtype_out, int ntime, int nsrc, int ntarg,
                                         long long ncol, const void *var, const void *ps, const double *ap,
                                         const double *b, const double *targ_plev, int extrapolate, int src_reversed,
                                         int out_reversed, void *out) {
    CHECK_COMMON(ctx, dtype_in, ntime, ncol);
    NEED(ctx, dtype_out == PGW_F64 || (dtype_out == PGW_F32 && dtype_in == PGW_F32), "dtype pair must be F32->F64, F64->F64 or F32->F32");
    NEED(ctx, nsrc >= 2 && nsrc <= MAX_NLEV, "nsrc must be in [2, 256]");
    NEED(ctx, ntarg >= 1 && ntarg <= MAX_TARG_PLEV, "ntarg must be in [1, 256]");
    NEED(ctx, var && ps && ap && b && targ_plev && out, "null pointer");
    if (extrapolate < 0 || extrapolate > 3) return fail(ctx, PGW_ERR_ARG, "Invalid input value for \"extrapolate\"");
    int rc = status_reset(ctx);
    if (rc) return rc;
    // ap | b | targ_plev -> the context's small device scratch (pageable source: the copy has left the caller's arrays on return)
    double *d_ap = ctx->d_small, *d_b = d_ap + MAX_NLEV, *d_plev = d_b + MAX_NLEV;
    HIPCHK(ctx, hipMemcpyAsync(d_ap, ap, sizeof(double) * nsrc, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(d_b, b, sizeof(double) * nsrc, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(d_plev, targ_plev, sizeof(double) * ntarg, hipMemcpyHostToDevice, ctx->stream));
    const size_t s_in = elem_size(dtype_in), s_out = elem_size(dtype_out);
    // columns per thread: the kernel is bound by instruction issue (about 95 logarithms and 99 interpolations per column),
    // not by its streams, and the second column's registers cost a wave per SIMD (122 -> 4 waves against 88 -> 5): same
    // box, S = 95, N = 99, 2 GB in, V = 2 / 1: 2.57 / 2.35 ms (float32 in), 1.40 / 1.30 ms (float64 in).  PGW_H2P_MAX_V = 2
    // compiles the two-column form in (16-B stores per lane); pick_vec then chooses it by shape and alignment.
    const int vec = pick_vec(ctx, dtype_in, ncol, {var, ps, out}, H2P_MAX_V);
    const unsigned long long big_in = (unsigned long long)ntime * nsrc * ncol * s_in, big_out = (unsigned long long)ntime * ntarg * ncol * s_out;
    const bool o32 = big_in < (1ull << 32) && big_out < (1ull << 32) && !ctx->opt[PGW_OPT_FORCE_OFF64];
    const int sr = src_reversed != 0, orv = out_reversed != 0;
    {
        Prof pr(ctx, PGW_K_HYBRID_TO_PLEV);
        auto launch = [&](auto ti_, auto to_) { with_offsets(o32, [&](auto o_) { with_int<4>(extrapolate, [&](auto m_) {
            using TI = decltype(ti_); using TO = decltype(to_); using O = decltype(o_);
            constexpr int M = decltype(m_)::value;
            auto form = [&](auto v_) {
                constexpr int V = decltype(v_)::value;
                hipLaunchKernelGGL((k_hybrid_to_plev<TI, TO, V, M, O>), dim3(nblocks((long long)ntime * ncol / V, BLOCK)), dim3(BLOCK), 0,
                                   ctx->stream, ntime, nsrc, ntarg, ncol, (const TI *)var, (const TI *)ps, d_ap, d_b, d_plev, sr, orv,
                                   (TO *)out, ctx->d_status);
            };
            if constexpr (H2P_MAX_V >= 2) { if (vec == 2) return form(int_c<H2P_MAX_V>()); }
            form(int_c<1>());
        }); }); };
        if (dtype_in == PGW_F64) launch(double(), double());
        else if (dtype_out == PGW_F64) launch(float(), double());
        else launch(float(), float());
    }
    HIPCHK(ctx, hipGetLastError());
    return status_check(ctx);
}

// ------------------------------------------------------------------ step_01: Emon hus -> hur
extern "C" int pgw_magnus_rh(pgw_ctx *ctx, int dtype, int ntime, int nplev, long long ncol, const void *qv,
                             const double *plev, const void *ta, double *rh) {
    CHECK_COMMON(ctx, dtype, ntime, ncol);
    NEED(ctx, nplev >= 1 && nplev <= MAX_TARG_PLEV, "nplev must be in [1, 256]");
    NEED(ctx, qv && plev && ta && rh, "null pointer");
    double *d_plev = ctx->d_small;
    HIPCHK(ctx, hipMemcpyAsync(d_plev, plev, sizeof(double) * nplev, hipMemcpyHostToDevice, ctx->stream));
    const long long n = (long long)ntime * nplev * ncol;
    const unsigned int nb = flat_grid(n);
    {
        Prof pr(ctx, PGW_K_MAGNUS_RH);
        with_type(dtype, [&](auto t_) {
            using T = decltype(t_);
            hipLaunchKernelGGL((k_magnus_rh<T>), dim3(nb), dim3(BLOCK), 0, ctx->stream, n, nplev, ncol, (const T *)qv, d_plev,
                               (const T *)ta, rh);
        });
    }
    HIPCHK(ctx, hipGetLastError());
    return PGW_OK;
}

extern "C" int pgw_hur_merge_levels(pgw_ctx *ctx, int dtype_amon, int ntime, int nplev, int namon, long long ncol,
                                    const double *hur, const void *amon, const int *copy_from, const int *e_above,
                                    const int *e_below, const int *a_above, const int *a_below, double *out) {
    CHECK_COMMON(ctx, dtype_amon, ntime, ncol);
    NEED(ctx, nplev >= 1 && nplev <= MAX_TARG_PLEV && namon >= 1, "nplev must be in [1, 256], namon positive");
    NEED(ctx, hur && amon && copy_from && e_above && e_below && a_above && a_below && out, "null pointer");
    NEED(ctx, hur != out, "out must not alias hur");
    std::vector<MergeLevel> tab(nplev);
    for (int l = 0; l < nplev; ++l) {
        MergeLevel m = {copy_from[l], e_above[l], e_below[l], a_above[l], a_below[l]};
        if (m.copy >= 0) NEED(ctx, m.copy < namon, "copy_from out of range");
        else NEED(ctx, m.e_above >= 0 && m.e_above < nplev && m.e_below >= 0 && m.e_below < nplev && m.a_above >= 0 &&
                       m.a_above < namon && m.a_below >= 0 && m.a_below < namon, "level table out of range");
        tab[l] = m;
    }
    MergeLevel *d_tab = (MergeLevel *)ctx->d_small;
    HIPCHK(ctx, hipMemcpyAsync(d_tab, tab.data(), sizeof(MergeLevel) * nplev, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));          // `tab` goes out of scope
    const long long n = (long long)ntime * nplev * ncol;
    const unsigned int nb = flat_grid(n);
    {
        Prof pr(ctx, PGW_K_HUR_MERGE);
        with_type(dtype_amon, [&](auto t_) {
            using T = decltype(t_);
            hipLaunchKernelGGL((k_hur_merge_levels<T>), dim3(nb), dim3(BLOCK), 0, ctx->stream, ntime, nplev, namon, ncol, hur,
                               (const T *)amon, d_tab, out);
        });
    }
    HIPCHK(ctx, hipGetLastError());
    return PGW_OK;
}

// ------------------------------------------------------------------ step_01: climatologies and their difference
// Shape of a launch over the records x (nrec, inner): cells per thread and the byte-offset type of x
struct ClimForm { int vec; bool o32; };
static ClimForm clim_form(pgw_ctx *ctx, int dtype_in, int nrec, long long inner, std::initializer_list<const void *> ptrs) {
    const unsigned long long big = (unsigned long long)nrec * (unsigned long long)inner * elem_size(dtype_in);
    return ClimForm{pick_vec(ctx, dtype_in, inner, ptrs), big < (1ull << 32) && !ctx->opt[PGW_OPT_FORCE_OFF64]};
}

extern "C" int pgw_clim_accumulate(pgw_ctx *ctx, int dtype_in, int dtype_out, int nrec, long long inner, const void *x,
                                   int first, int last, double *sum, int *cnt, void *mean) {
    CHECK_COMMON(ctx, dtype_in, nrec, inner);
    NEED(ctx, dtype_out == dtype_in || dtype_out == PGW_F64, "dtype_out must be dtype_in or PGW_F64");
    NEED(ctx, x, "null pointer");
    const bool carried = !(first && last);
    NEED(ctx, !carried || (sum && cnt), "sum and cnt are needed unless first and last are both set");
    NEED(ctx, !last || mean, "mean is needed with last");
    const ClimForm f = clim_form(ctx, dtype_in, nrec, inner, {x, carried ? sum : nullptr, carried ? cnt : nullptr, last ? mean : nullptr});
    {
        Prof pr(ctx, PGW_K_CLIM_ACCUMULATE);
        auto launch = [&](auto ti_, auto to_) { with_offsets(f.o32, [&](auto o_) {
            using TI = decltype(ti_); using TO = decltype(to_); using O = decltype(o_);
            auto form = [&](auto v_) {
                constexpr int V = decltype(v_)::value;
                hipLaunchKernelGGL((k_clim_accumulate<TI, TO, V, O>), dim3(nblocks(inner / V, BLOCK)), dim3(BLOCK), 0, ctx->stream, nrec,
                                   inner, (const TI *)x, first ? 1 : 0, last ? 1 : 0, sum, cnt, (TO *)mean);
            };
            if constexpr (sizeof(TI) == 8) { if (f.vec >= 2) form(int_c<2>()); else form(int_c<1>()); }
            else with_vec(f.vec, form);
        }); };
        if (dtype_in == PGW_F64) launch(double(), double());
        else if (dtype_out == PGW_F64) launch(float(), double());
        else launch(float(), float());
    }
    HIPCHK(ctx, hipGetLastError());
    return PGW_OK;
}

extern "C" int pgw_test_read_records(pgw_ctx *ctx, int dtype, int nrec, long long inner, const void *x) {
    CHECK_COMMON(ctx, dtype, nrec, inner);
    NEED(ctx, x, "null pointer");
    const ClimForm f = clim_form(ctx, dtype, nrec, inner, {x});
    {
        Prof pr(ctx, PGW_K_CLIM_READ);
        with_type_vec(dtype, f.vec, [&](auto t_, auto v_) { with_offsets(f.o32, [&](auto o_) {
            using T = decltype(t_); using O = decltype(o_);
            constexpr int V = decltype(v_)::value;
            hipLaunchKernelGGL((k_clim_read<T, V, O>), dim3(nblocks(inner / V, BLOCK)), dim3(BLOCK), 0, ctx->stream, nrec, inner,
                               (const T *)x, (T *)nullptr);
        }); });
    }
    HIPCHK(ctx, hipGetLastError());
    return PGW_OK;
}

// postproc_cosmo/extpar_adapt.py:20-32: out = base + time mean of x where base is not a mask value (k_time_mean_add)
extern "C" int pgw_time_mean_add(pgw_ctx *ctx, int dtype_base, int dtype_x, int nrec, long long n, const void *base, int nmask,
                                 const double *mask_values, const void *x, void *out, void *mean, long long *n_masked,
                                 long long *n_new_nan) {
    NEED(ctx, TAG_OK(dtype_base), "dtype_base must be PGW_F32 or PGW_F64");
    CHECK_COMMON(ctx, dtype_x, nrec, n);
    NEED(ctx, x, "null pointer");
    NEED(ctx, (base != nullptr) == (out != nullptr), "base and out must be given together");
    NEED(ctx, nmask >= 0 && nmask <= 2 && (nmask == 0 || mask_values), "nmask must be in [0, 2]");
    MeanAddMask mk = {nmask, {0.0, 0.0}};
    for (int k = 0; k < nmask; ++k) mk.v[k] = dtype_base == PGW_F32 ? (double)(float)mask_values[k] : mask_values[k];
    const ClimForm f = clim_form(ctx, dtype_x, nrec, n, {x, base, out, mean});
    unsigned long long *d_cnt = (unsigned long long *)ctx->d_small, h_cnt[2] = {0, 0};
    HIPCHK(ctx, hipMemsetAsync(d_cnt, 0, sizeof(h_cnt), ctx->stream));
    if (n == 1) with_type(dtype_base, [&](auto b_) { with_type(dtype_x, [&](auto x_) {     // one cell: numpy's pairwise order
        using TB = decltype(b_); using TX = decltype(x_);
        hipLaunchKernelGGL((k_time_mean_add_one<TX, TB>), dim3(1), dim3(64), 0, ctx->stream, nrec, (const TB *)base, mk,
                           (const TX *)x, (TB *)out, (TX *)mean, d_cnt);
    }); });
    else with_type(dtype_base, [&](auto b_) { with_type_vec(dtype_x, f.vec, [&](auto x_, auto v_) { with_offsets(f.o32, [&](auto o_) {
        using TB = decltype(b_); using TX = decltype(x_); using O = decltype(o_);
        constexpr int V = decltype(v_)::value;
        hipLaunchKernelGGL((k_time_mean_add<TX, TB, V, O>), dim3(nblocks(n / V, BLOCK)), dim3(BLOCK), 0, ctx->stream, nrec, n,
                           (const TB *)base, mk, (const TX *)x, (TB *)out, (TX *)mean, d_cnt);
    }); }); });
    HIPCHK(ctx, hipGetLastError());
    HIPCHK(ctx, hipMemcpyAsync(h_cnt, d_cnt, sizeof(h_cnt), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    if (n_masked) *n_masked = (long long)h_cnt[0];
    if (n_new_nan) *n_new_nan = (long long)h_cnt[1];
    return PGW_OK;
}

extern "C" int pgw_field_sub(pgw_ctx *ctx, int dtype, long long n, const void *a, const void *b, void *out) {
    NEED(ctx, dtype == PGW_F32 || dtype == PGW_F64, "dtype must be PGW_F32 or PGW_F64");
    NEED(ctx, n >= 1 && a && b && out, "bad argument");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    int vec = pick_vec(ctx, dtype, n, {a, b, out});
    const unsigned int nb = flat_grid(n / vec);
    {
        Prof pr(ctx, PGW_K_FIELD_SUB);
        with_type_vec(dtype, vec, [&](auto t_, auto v_) {
            using T = decltype(t_);
            hipLaunchKernelGGL((k_field_sub<T, decltype(v_)::value>), dim3(nb), dim3(BLOCK), 0, ctx->stream, n, (const T *)a,
                               (const T *)b, (T *)out);
        });
    }
    HIPCHK(ctx, hipGetLastError());
    return PGW_OK;
}

// ------------------------------------------------------------------ hydrostatic check: geopotential on pressure levels
// The level list in descending pressure with the permutation back to the caller's order (stable: equal levels keep the
// caller's order), logarithms from the device table like plev_table's.
static int geo_targets(pgw_ctx *ctx, int nplev, const double *plev, GeoTargets *gt) {
    memset(gt, 0, sizeof(*gt));
    gt->n = nplev;
    for (int i = 0; i < nplev; ++i) {
        if (!(plev[i] > 0.0001 && plev[i] <= 1.7976931348623157e308))             // :135 guard value; NaN fails too
            return fail(ctx, PGW_ERR_ARG, "pgw_geopot_on_plev: plev[%d] = %g must be finite and greater than 1e-4", i, plev[i]);
        gt->row[i] = i;
    }
    std::stable_sort(gt->row, gt->row + nplev, [&](int a, int b) { return plev[a] > plev[b]; });
    for (int i = 0; i < nplev; ++i) gt->p[i] = plev[gt->row[i]];
    double *d_in = ctx->d_small, *d_out = ctx->d_small + MAX_PLEV;
    HIPCHK(ctx, hipMemcpyAsync(d_in, gt->p, sizeof(double) * nplev, hipMemcpyHostToDevice, ctx->stream));
    hipLaunchKernelGGL(k_log_table, dim3(1), dim3(64), 0, ctx->stream, nplev, d_in, d_out);
    HIPCHK(ctx, hipMemcpyAsync(gt->lnp, d_out, sizeof(double) * nplev, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return PGW_OK;
}

extern "C" int pgw_geopot_on_plev(pgw_ctx *ctx, int dtype_2d, int dtype_a, int dtype_b, int ntime, int nplev, long long ncol,
                                  const double *plev, const void *FIS, const void *PS_a, const void *T_a, const void *QV_a,
                                  const void *PS_b, const void *T_b, const void *QV_b, int dtype_zg, const void *zg_before,
                                  const void *zg_after, double x_hi, double x_new, double g, int form, double *out,
                                  long long *nan_count) {
    CHECK_COMMON(ctx, dtype_2d, ntime, ncol);
    NEED(ctx, ctx->nlev > 0, "pgw_set_levels has not been called");
    NEED(ctx, TAG_OK(dtype_a), "dtype_a must be PGW_F32 or PGW_F64");
    NEED(ctx, nplev >= 1 && nplev <= MAX_PLEV && plev, "nplev must be in [1, 64]");
    NEED(ctx, FIS && PS_a && T_a && QV_a && out, "null pointer");
    const bool two = PS_b != nullptr;
    NEED(ctx, two == (T_b != nullptr) && two == (QV_b != nullptr), "PS_b, T_b and QV_b must be given together");
    NEED(ctx, !two || TAG_OK(dtype_b), "dtype_b must be PGW_F32 or PGW_F64");
    NEED(ctx, !zg_before || two, "a zg record needs two states");
    NEED(ctx, !zg_before || TAG_OK(dtype_zg), "dtype_zg must be PGW_F32 or PGW_F64");
    NEED(ctx, !zg_before || x_hi == 0.0 || zg_after, "zg_after is needed unless x_hi is 0");
    NEED(ctx, form == 0 || form == 1, "form must be 0 (one walk) or 1 (two walks)");
    for (const void *p : {FIS, PS_a, T_a, QV_a, PS_b, T_b, QV_b, zg_before, zg_after})
        NEED(ctx, p != (const void *)out, "out must not be one of the inputs");
    GeoTargets gt;
    int rc = geo_targets(ctx, nplev, plev, &gt);
    if (rc) return rc;
    unsigned long long *d_cnt = (unsigned long long *)(ctx->d_small + 2 * MAX_PLEV);
    HIPCHK(ctx, hipMemsetAsync(d_cnt, 0, sizeof(unsigned long long) * MAX_PLEV, ctx->stream));
    ZgDelta zg = {zg_before, (zg_before && x_hi != 0.0) ? zg_after : nullptr, dtype_zg == PGW_F32 ? 1 : 0, x_hi, x_new, g};
    const Levels lv = levels_of(ctx);
    const unsigned int nb = nblocks((long long)ntime * ncol, BLOCK);
    {
        Prof pr(ctx, PGW_K_INTEG_GEOPOT);
        with_type(dtype_2d, [&](auto t2_) { with_type(dtype_a, [&](auto ta_) {
            using T2 = decltype(t2_); using TLA = decltype(ta_);
            if (!two) {
                hipLaunchKernelGGL((k_geopot_plev<T2, TLA, TLA, 1, false>), dim3(nb), dim3(BLOCK), 0, ctx->stream, gt, lv, ntime, ncol,
                                   (const T2 *)FIS, (const T2 *)PS_a, (const TLA *)T_a, (const TLA *)QV_a, (const T2 *)nullptr,
                                   (const TLA *)nullptr, (const TLA *)nullptr, zg, out, d_cnt);
                return;
            }
            with_type(dtype_b, [&](auto tb_) { with_int<2>(form, [&](auto f_) {
                using TLB = decltype(tb_);
                hipLaunchKernelGGL((k_geopot_plev<T2, TLA, TLB, 2, decltype(f_)::value == 0>), dim3(nb), dim3(BLOCK), 0, ctx->stream, gt,
                                   lv, ntime, ncol, (const T2 *)FIS, (const T2 *)PS_a, (const TLA *)T_a, (const TLA *)QV_a,
                                   (const T2 *)PS_b, (const TLB *)T_b, (const TLB *)QV_b, zg, out, d_cnt);
            }); });
        }); });
    }
    HIPCHK(ctx, hipGetLastError());
    if (nan_count) {
        unsigned long long h[MAX_PLEV];
        HIPCHK(ctx, hipMemcpyAsync(h, d_cnt, sizeof(h), hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
        for (int i = 0; i < nplev; ++i) nan_count[i] = (long long)h[i];            // the kernel counts by output row
    }
    return PGW_OK;
}

extern "C" int pgw_level_stats(pgw_ctx *ctx, int nrow, long long ncol, const double *x, long long *count, double *sum,
                               double *sumsq, double *maxabs) {
    NEED(ctx, nrow >= 1 && nrow <= 65535 && ncol >= 1, "nrow must be in [1, 65535], ncol positive");
    NEED(ctx, x && count && sum && sumsq && maxabs, "null pointer");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    unsigned int nbx = nblocks(ncol, BLOCK * 8);                  // a function of the shape alone
    if (nbx > 64) nbx = 64;
    void *part = nullptr;
    const size_t bytes = sizeof(double) * 4 * nbx * (size_t)nrow;
    int rc = ws_get(ctx, 7, bytes, &part);
    if (rc) return rc;
    hipLaunchKernelGGL(k_level_stats, dim3(nbx, nrow), dim3(BLOCK), 0, ctx->stream, ncol, x, (double *)part);
    HIPCHK(ctx, hipGetLastError());
    std::vector<double> h((size_t)4 * nbx * nrow);
    HIPCHK(ctx, hipMemcpyAsync(h.data(), part, bytes, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    for (int r = 0; r < nrow; ++r) {
        double c = 0.0, s = 0.0, q = 0.0, m = 0.0;
        for (unsigned int b = 0; b < nbx; ++b) {                  // the blocks of a row in the order of their index
            const double *p = h.data() + ((size_t)r * nbx + b) * 4;
            c += p[0]; s += p[1]; q += p[2]; m = p[3] > m ? p[3] : m;
        }
        count[r] = (long long)c; sum[r] = s; sumsq[r] = q; maxabs[r] = m;
    }
    return PGW_OK;
}

// ------------------------------------------------------------------ delta check: T, RH, U, V on pressure levels
extern "C" int pgw_state_on_plev(pgw_ctx *ctx, int dtype_2d, int dtype_a, int dtype_b, int ntime, int nplev, long long ncol,
                                 const double *plev, const void *PS_a, const void *T_a, const void *QV_a, const void *U_a,
                                 const void *V_a, const void *PS_b, const void *T_b, const void *QV_b, const void *U_b,
                                 const void *V_b, int dtype_delta, const void *const *rec_before, const void *const *rec_after,
                                 const void *ps_hist_before, const void *ps_hist_after, const double *x_hi, const double *x_new,
                                 double *out, double *out_error) {
    // every check comes before the first upload or launch
    NEED(ctx, TAG_OK(dtype_2d) && TAG_OK(dtype_a), "dtype_2d and dtype_a must be PGW_F32 or PGW_F64");
    NEED(ctx, ntime >= 1 && ncol >= 1, "ntime and ncol must be positive");
    NEED(ctx, ctx->nlev > 0, "pgw_set_levels has not been called");
    NEED(ctx, nplev >= 1 && nplev <= MAX_PLEV_WIDE, "nplev must be in [1, 128]");
    static_assert(MAX_PLEV_WIDE == 128, "the message above names the limit");
    NEED(ctx, plev && PS_a && T_a && QV_a && U_a && V_a && out, "null pointer");
    for (int i = 0; i < nplev; ++i)
        if (!(plev[i] > 0.0001 && plev[i] <= 1.7976931348623157e308))
            return fail(ctx, PGW_ERR_ARG, "pgw_state_on_plev: plev[%d] = %g must be finite and greater than 1e-4", i, plev[i]);
    const int nb_given = (PS_b != nullptr) + (T_b != nullptr) + (QV_b != nullptr) + (U_b != nullptr) + (V_b != nullptr);
    NEED(ctx, nb_given == 0 || nb_given == 5, "PS_b, T_b, QV_b, U_b and V_b must be given together");
    const bool two = nb_given == 5;
    NEED(ctx, !two || TAG_OK(dtype_b), "dtype_b must be PGW_F32 or PGW_F64");
    auto aligned = [](const void *p, size_t s) { return ((uintptr_t)p % s) == 0; };
    const size_t s2 = elem_size(dtype_2d), sa = elem_size(dtype_a), sb = two ? elem_size(dtype_b) : 1;
    NEED(ctx, aligned(PS_a, s2) && aligned(T_a, sa) && aligned(QV_a, sa) && aligned(U_a, sa) && aligned(V_a, sa) && aligned(PS_b, s2) &&
                  aligned(T_b, sb) && aligned(QV_b, sb) && aligned(U_b, sb) && aligned(V_b, sb) && aligned(out, 8) && aligned(out_error, 8),
         "a pointer is not aligned to its element");
    PlevRecords rec;
    memset(&rec, 0, sizeof(rec));
    if (out_error) {
        NEED(ctx, two, "out_error needs two states");
        NEED(ctx, TAG_OK(dtype_delta), "dtype_delta must be PGW_F32 or PGW_F64");
        NEED(ctx, rec_before && rec_after && x_hi && x_new && ps_hist_before && ps_hist_after, "out_error needs the record pointers");
        const size_t sd = elem_size(dtype_delta);
        for (int v = 0; v < 4; ++v) {
            NEED(ctx, rec_before[v] && rec_after[v], "out_error needs all ten record pointers");
            NEED(ctx, aligned(rec_before[v], sd) && aligned(rec_after[v], sd), "a pointer is not aligned to its element");
            NEED(ctx, rec_before[v] != (const void *)out && rec_after[v] != (const void *)out, "out must not be one of the inputs");
            rec.b[v] = rec_before[v]; rec.a[v] = x_hi[v] == 0.0 ? nullptr : rec_after[v];
        }
        NEED(ctx, aligned(ps_hist_before, sd) && aligned(ps_hist_after, sd), "a pointer is not aligned to its element");
        NEED(ctx, out_error != out, "out_error must not be out");
        rec.ps_b = ps_hist_before; rec.ps_a = x_hi[4] == 0.0 ? nullptr : ps_hist_after;
        for (int v = 0; v < 5; ++v) { rec.x_hi[v] = x_hi[v]; rec.x_new[v] = x_new[v]; }
        rec.f32 = dtype_delta == PGW_F32 ? 1 : 0;
    }
    for (const void *p : {PS_a, T_a, QV_a, U_a, V_a, PS_b, T_b, QV_b, U_b, V_b})
        NEED(ctx, p != (const void *)out && (!out_error || p != (const void *)out_error), "an output must not be one of the inputs");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    // the list in ascending pressure with the permutation back to the caller's rows (stable: repeats keep their order)
    int row[MAX_PLEV_WIDE];
    double sorted[MAX_PLEV_WIDE];
    for (int i = 0; i < nplev; ++i) row[i] = i;
    std::stable_sort(row, row + nplev, [&](int a, int b) { return plev[a] < plev[b]; });
    for (int i = 0; i < nplev; ++i) sorted[i] = plev[row[i]];
    static_assert(MAX_PLEV_WIDE * (sizeof(double) + sizeof(int)) <= SMALL_BYTES, "d_small holds the level list and its rows");
    double *d_plev = ctx->d_small;
    int *d_row = (int *)(ctx->d_small + MAX_PLEV_WIDE);
    HIPCHK(ctx, hipMemcpyAsync(d_plev, sorted, sizeof(double) * nplev, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(d_row, row, sizeof(int) * nplev, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));           // `sorted` and `row` go out of scope
    const unsigned long long cells = (unsigned long long)ntime * (unsigned long long)ncol;
    const unsigned long long big_in = cells * ctx->nlev * 8ull, big_out = 4ull * cells * nplev * sizeof(double);
    const bool o32 = big_in < (1ull << 32) && big_out < (1ull << 32) && !ctx->opt[PGW_OPT_FORCE_OFF64];
    const Levels lv = levels_of(ctx);
    const unsigned int nb = nblocks((long long)cells, BLOCK);
    {
        Prof pr(ctx, PGW_K_HYBRID_TO_PLEV);
        with_type(dtype_2d, [&](auto t2_) { with_type(dtype_a, [&](auto ta_) { with_offsets(o32, [&](auto o_) {
            using T2 = decltype(t2_); using TLA = decltype(ta_); using O = decltype(o_);
            if (!two) {
                hipLaunchKernelGGL((k_state_plev<T2, TLA, TLA, 1, O>), dim3(nb), dim3(BLOCK), 0, ctx->stream, lv, ntime, nplev, ncol,
                                   d_plev, d_row, (const T2 *)PS_a, (const TLA *)T_a, (const TLA *)QV_a, (const TLA *)U_a,
                                   (const TLA *)V_a, (const T2 *)nullptr, (const TLA *)nullptr, (const TLA *)nullptr,
                                   (const TLA *)nullptr, (const TLA *)nullptr, rec, out, (double *)nullptr);
                return;
            }
            with_type(dtype_b, [&](auto tb_) {
                using TLB = decltype(tb_);
                hipLaunchKernelGGL((k_state_plev<T2, TLA, TLB, 2, O>), dim3(nb), dim3(BLOCK), 0, ctx->stream, lv, ntime, nplev, ncol,
                                   d_plev, d_row, (const T2 *)PS_a, (const TLA *)T_a, (const TLA *)QV_a, (const TLA *)U_a,
                                   (const TLA *)V_a, (const T2 *)PS_b, (const TLB *)T_b, (const TLB *)QV_b, (const TLB *)U_b,
                                   (const TLB *)V_b, rec, out, out_error);
            });
        }); }); });
    }
    HIPCHK(ctx, hipGetLastError());
    return PGW_OK;
}

// ------------------------------------------------------------------ step_01: level list, lon-lat box, model-top merge
extern "C" int pgw_select_box(pgw_ctx *ctx, int elem_bytes, int nrec, int nlev_src, int nlat_src, int nlon_src, const void *src,
                              int nlev_sel, const int *lev_index, int lat0, int nlat_sel, int lon0, int nlon_sel, int nlev_dst,
                              int lev_dst0, void *dst) {
    NEED(ctx, elem_bytes == 2 || elem_bytes == 4 || elem_bytes == 8, "elem_bytes must be 2, 4 or 8");
    NEED(ctx, nrec >= 1 && nlev_src >= 1 && nlat_src >= 1 && nlon_src >= 1, "nrec, nlev_src, nlat_src and nlon_src must be positive");
    NEED(ctx, src && dst, "null pointer");
    NEED(ctx, nlev_sel >= 1 && nlev_sel <= SEL_MAX_LEVELS, "nlev_sel must be in [1, 256]");
    NEED(ctx, lev_index || nlev_sel <= nlev_src, "without lev_index nlev_sel must not exceed nlev_src");
    SelLevels tab;
    for (int k = 0; k < nlev_sel; ++k) {
        tab.lev[k] = lev_index ? lev_index[k] : k;
        NEED(ctx, tab.lev[k] >= 0 && tab.lev[k] < nlev_src, "lev_index must lie in [0, nlev_src)");
    }
    NEED(ctx, lat0 >= 0 && nlat_sel >= 1 && (long long)lat0 + nlat_sel <= nlat_src, "lat0 .. lat0 + nlat_sel must lie within [0, nlat_src]");
    NEED(ctx, lon0 >= 0 && lon0 < nlon_src, "lon0 must lie in [0, nlon_src)");
    NEED(ctx, nlon_sel >= 1 && nlon_sel <= nlon_src, "nlon_sel must be in [1, nlon_src]");
    NEED(ctx, lev_dst0 >= 0 && nlev_dst >= 1 && (long long)lev_dst0 + nlev_sel <= nlev_dst, "lev_dst0 + nlev_sel must not exceed nlev_dst");
    const unsigned long long eb = (unsigned long long)elem_bytes;
    const unsigned long long src_bytes = (unsigned long long)nrec * nlev_src * nlat_src * nlon_src * eb;
    const unsigned long long dst_bytes = (unsigned long long)nrec * nlev_dst * nlat_sel * nlon_sel * eb;
    const uintptr_t ps = (uintptr_t)src, pd = (uintptr_t)dst;
    NEED(ctx, ps % eb == 0 && pd % eb == 0, "src and dst must be aligned to elem_bytes");
    NEED(ctx, ps + src_bytes <= pd || pd + dst_bytes <= ps, "src and dst must not overlap");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    // bytes per lane: the widest word (16, 8, 4, 2) that divides both row lengths, the first column - and with it the place
    // where the window wraps, nlon_src - lon0 - and both base addresses; every row then starts on such a word
    unsigned long long wb = ctx->opt[PGW_OPT_FORCE_VEC1] ? eb : 16;
    while (wb > eb && ((nlon_src * eb) % wb || (nlon_sel * eb) % wb || (lon0 * eb) % wb || ps % wb || pd % wb)) wb >>= 1;
    const unsigned long long per = wb / eb, nsel_w = (unsigned long long)nlon_sel / per;
    const unsigned int lpr = (unsigned int)std::min<unsigned long long>(nsel_w, BLOCK), rpb = BLOCK / lpr;
    const unsigned long long nrows = (unsigned long long)nrec * nlev_sel * nlat_sel;
    const unsigned long long tile_rows = (unsigned long long)rpb * SEL_ROWS;
    const unsigned int grid = (unsigned int)std::min<unsigned long long>((nrows + tile_rows - 1) / tile_rows, 256ull * 16);
    const bool o32 = src_bytes < (1ull << 32) && dst_bytes < (1ull << 32) && !ctx->opt[PGW_OPT_FORCE_OFF64];
    with_offsets(o32, [&](auto o_) {
        using O = decltype(o_);
        const SelBox<O> a = {(O)nrows, (unsigned int)nlev_sel, (unsigned int)nlat_sel, (O)nlev_src, (O)nlat_src,
                             (O)((unsigned long long)nlon_src / per), (O)lat0, (O)((unsigned long long)lon0 / per), (O)nsel_w,
                             (O)nlev_dst, (O)lev_dst0, lpr, rpb};
        auto launch = [&](auto w_) {
            using W = decltype(w_);
            hipLaunchKernelGGL((k_select_box<W, O>), dim3(grid), dim3(BLOCK), 0, ctx->stream, a, tab, (const W *)src, (W *)dst);
        };
        if (wb == 16) launch(VecOf<unsigned int, 4>::type());
        else if (wb == 8) launch((unsigned long long)0);
        else if (wb == 4) launch((unsigned int)0);
        else launch((unsigned short)0);
    });
    HIPCHK(ctx, hipGetLastError());
    return PGW_OK;
}

// ------------------------------------------------------------------ step_01: lon-lat box on a curvilinear grid
extern "C" int pgw_box_mark_2d(pgw_ctx *ctx, int dtype, int nj, int ni, const void *lat, const void *lon, double lon1, double lon2,
                               double lat1, double lat2, int *row_any, int *col_any, long long *n_inside) {
    NEED(ctx, TAG_OK(dtype), "dtype must be PGW_F32 or PGW_F64");
    NEED(ctx, nj >= 1 && ni >= 1, "nj and ni must be positive");
    NEED(ctx, (long long)nj * ni < (1ll << 31), "nj * ni must be below 2^31 cells");
    NEED(ctx, lat && lon && row_any && col_any && n_inside, "null pointer");
    NEED(ctx, lon1 == lon1 && lon2 == lon2 && lat1 == lat1 && lat2 == lat2, "the box must not hold a NaN");
    NEED(ctx, lon1 < lon2 && lon2 - lon1 <= 360.0, "the box needs lon1 < lon2 and lon2 - lon1 <= 360");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const long long n = (long long)nj * ni;
    const BoxMark b = {lon1, lon2, lat1 < lat2 ? lat1 : lat2, lat1 < lat2 ? lat2 : lat1};
    HIPCHK(ctx, hipMemsetAsync(row_any, 0, sizeof(int) * (size_t)nj, ctx->stream));
    HIPCHK(ctx, hipMemsetAsync(col_any, 0, sizeof(int) * (size_t)ni, ctx->stream));
    HIPCHK(ctx, hipMemsetAsync(n_inside, 0, sizeof(long long), ctx->stream));
    with_type(dtype, [&](auto t_) {
        using T = decltype(t_);
        hipLaunchKernelGGL((k_box_mark_2d<T>), dim3(nblocks(n, BLOCK)), dim3(BLOCK), 0, ctx->stream, n, ni, b, (const T *)lat,
                           (const T *)lon, row_any, col_any, (unsigned long long *)n_inside);
    });
    HIPCHK(ctx, hipGetLastError());
    return PGW_OK;
}

// ------------------------------------------------------------------ time lerp
extern "C" int pgw_time_lerp(pgw_ctx *ctx, int dtype, long long n, const void *v_before, const void *v_after,
                             double x_hi, double x_new, void *out) {
    NEED(ctx, dtype == PGW_F32 || dtype == PGW_F64, "dtype must be PGW_F32 or PGW_F64");
    NEED(ctx, n >= 1 && v_before && v_after && out, "bad argument");
    int vec = pick_vec(ctx, dtype, n, {v_before, v_after, out});
    const unsigned int nb = flat_grid(n / vec);
    {
        Prof pr(ctx, PGW_K_TIME_LERP);
        with_type_vec(dtype, vec, [&](auto t_, auto v_) {
            using T = decltype(t_);
            hipLaunchKernelGGL((k_time_lerp<T, decltype(v_)::value>), dim3(nb), dim3(BLOCK), 0, ctx->stream, n, (const T *)v_before,
                               (const T *)v_after, x_hi, x_new, (T *)out);
        });
    }
    HIPCHK(ctx, hipGetLastError());
    return PGW_OK;
}

// ------------------------------------------------------------------ vert_interp_delta
// The first MAX_PLEV entries of a table as a narrow one (all of it when n <= MAX_PLEV; the unused entries of both are 0)
static PlevTable narrow_table(const PlevTableWide &w) {
    PlevTable t;
    memset(&t, 0, sizeof(t));
    memcpy(t.p, w.p, sizeof(t.p));
    memcpy(t.lnp, w.lnp, sizeof(t.lnp));
    t.pmax = w.pmax; t.pmin = w.pmin; t.n = w.n;
    return t;
}

// f(table) with the table type the axis needs: PlevTable for up to MAX_PLEV levels - the instantiations every such
// caller has always launched - and PlevTableWide above.  The callers have checked n <= MAX_PLEV_WIDE.
template <typename F>
static void with_plev(const PlevTableWide &w, F &&f) {
    if (w.n > MAX_PLEV) f(w);
    else f(narrow_table(w));
}
template <typename F>
static void with_plev(pgw_ctx *ctx, F &&f) {
    if (ctx->plev_tab_wide.n > MAX_PLEV) f(ctx->plev_tab_wide);
    else f(ctx->plev_tab);
}
// the error texts take the limit from the header's constant, which is the kernels'
#define PGW_STR2(x) #x
#define PGW_STR(x) PGW_STR2(x)
#define PLEV_RANGE_2 "nplev must be in [2, " PGW_STR(PGW_MAX_PLEV) "]"
#define PLEV_RANGE_1 "nplev must be in [1, " PGW_STR(PGW_MAX_PLEV) "]"
static_assert(MAX_PLEV_WIDE == PGW_MAX_PLEV && MAX_PLEV == PGW_MAX_PLEV_ZG, "include/pgw_hip.h names the kernels' limits");

// The plev axis of zg for the local reference level of a file: its own (nplev_zg, plev_zg) when given, else the deltas'.
// Its table stays narrow (LocalPRef, k_local_p_ref).
struct ZgAxis { int n; const double *plev; };
static int zg_axis(pgw_ctx *ctx, const pgw_file_args *a, ZgAxis *z) {
    NEED(ctx, a->nplev_zg >= 0 && a->nplev_zg <= MAX_PLEV, "nplev_zg must be in [1, " PGW_STR(PGW_MAX_PLEV_ZG) "], or 0 when zg shares plev");
    NEED(ctx, a->nplev_zg == 0 || a->plev_zg != nullptr, "plev_zg is NULL");
    z->n = a->nplev_zg ? a->nplev_zg : a->nplev;
    z->plev = a->nplev_zg ? a->plev_zg : a->plev;
    NEED(ctx, z->n <= MAX_PLEV, "local_p_ref: zg's plev axis must have at most " PGW_STR(PGW_MAX_PLEV_ZG) " levels (give nplev_zg / plev_zg when nplev is larger)");
    return PGW_OK;
}

static int plev_table(pgw_ctx *ctx, int nplev, const double *plev) {
    if ((int)ctx->plev_key.size() == nplev && memcmp(ctx->plev_key.data(), plev, sizeof(double) * nplev) == 0)
        return PGW_OK;
    ctx->plev_key.clear();
    PlevTableWide &t = ctx->plev_tab_wide;
    memset(&t, 0, sizeof(t));
    t.n = nplev;
    t.pmax = -INFINITY; t.pmin = INFINITY;
    bool anynan = false;
    for (int i = 0; i < nplev; ++i) {
        t.p[i] = plev[nplev - 1 - i];                       // functions.py:383-384 reversal
        if (t.p[i] != t.p[i]) anynan = true;
        if (t.p[i] > t.pmax) t.pmax = t.p[i];
        if (t.p[i] < t.pmin) t.pmin = t.p[i];
    }
    if (anynan) return fail(ctx, PGW_ERR_ARG, "vert_interp_delta: NaN in plev");
    // ln(plev) with the device log so that table and per-column logs are from one implementation
    static_assert(2 * MAX_PLEV_WIDE * sizeof(double) <= SMALL_BYTES, "d_small holds the table and its logarithms");
    double *d_in = ctx->d_small, *d_out = ctx->d_small + MAX_PLEV_WIDE;
    HIPCHK(ctx, hipMemcpyAsync(d_in, t.p, sizeof(double) * nplev, hipMemcpyHostToDevice, ctx->stream));
    // one entry per thread, blocks of 64: a second block for the levels past the 64th
    hipLaunchKernelGGL(k_log_table, dim3(nblocks(nplev, 64)), dim3(64), 0, ctx->stream, nplev, d_in, d_out);
    HIPCHK(ctx, hipMemcpyAsync(t.lnp, d_out, sizeof(double) * nplev, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    ctx->plev_tab = narrow_table(t);
    ctx->plev_key.assign(plev, plev + nplev);
    return PGW_OK;
}

// functions.py:417-425 on the minima a delta kernel left in the status block (already fetched by status_check):
// np.min(target_P) < np.min(source_P); NaN in either -> comparison False
static int top_pressure_check(pgw_ctx *ctx, int ignore_top) {
    if (!ignore_top) {
        DevStatus *h = ctx->h_status;
        if (!h->nan_seen && h->min_targ_bits != ~0ull && h->min_src_bits != ~0ull) {
            double mt, ms;
            memcpy(&mt, &h->min_targ_bits, 8);
            memcpy(&ms, &h->min_src_bits, 8);
            if (mt < ms) return fail_status(ctx, PGW_ERR_TOP_PRESSURE);
        }
    }
    return PGW_OK;
}

extern "C" int pgw_vert_interp_delta(pgw_ctx *ctx, int dtype, int ntime, int nplev, int nlev_t, long long ncol,
                                     const double *plev, const void *delta_b, const void *delta_a, double x_hi,
                                     double x_new, const void *dsfc_b, const void *dsfc_a, const void *pshist_b,
                                     const void *pshist_a, const void *targ_P, const void *ps, int ignore_top,
                                     const void *add_to, void *out) {
    CHECK_COMMON(ctx, dtype, ntime, ncol);
    NEED(ctx, nplev >= 2 && nplev <= MAX_PLEV_WIDE, PLEV_RANGE_2);
    NEED(ctx, plev && delta_b && out, "null pointer");
    NEED(ctx, targ_P || ps, "need targ_P or ps");
    NEED(ctx, (dsfc_b == nullptr) == (pshist_b == nullptr), "delta_sfc and ps_hist must be given together");
    if (!targ_P) {
        NEED(ctx, ctx->nlev > 0, "pgw_set_levels has not been called");
        NEED(ctx, nlev_t == ctx->nlev, "nlev_t must equal the context's nlev when targ_P is NULL");
    }
    NEED(ctx, nlev_t >= 1, "nlev_t must be positive");
    int rc = plev_table(ctx, nplev, plev);
    if (rc) return rc;
    rc = status_reset(ctx);
    if (rc) return rc;
    Levels lv = levels_of(ctx);
    if (targ_P) { lv.akm = lv.bkm = nullptr; }
    long long total = (long long)ntime * ncol;
    {
        Prof pr(ctx, PGW_K_VERT_INTERP_DELTA);
        with_type(dtype, [&](auto t_) { with_int<2>(dsfc_b != nullptr, [&](auto sfc_) { with_plev(ctx, [&](const auto &pt) {
            using T = decltype(t_); using PT = std::decay_t<decltype(pt)>;
            hipLaunchKernelGGL((k_vert_interp_delta<T, T, T, decltype(sfc_)::value != 0, T, T, T, PT>), dim3(nblocks(total, BLOCK)), dim3(BLOCK), 0,
                               ctx->stream, pt, lv, ntime, nlev_t, ncol, delta_src<T>(delta_b, delta_a, x_hi, x_new),
                               delta_src<T>(dsfc_b, dsfc_a, x_hi, x_new), delta_src<T>(pshist_b, pshist_a, x_hi, x_new),
                               (const T *)targ_P, (const T *)ps, ignore_top ? 0 : 1, (const T *)add_to, (T *)out, ctx->d_status);
        }); }); });
    }
    HIPCHK(ctx, hipGetLastError());
    rc = status_check(ctx);
    if (rc) return rc;
    return top_pressure_check(ctx, ignore_top);
}

// step_03 --debug_mode interpolate_full: the four deltas of load_delta_interp on the model levels of `ps`, one launch
extern "C" int pgw_delta_fields(pgw_ctx *ctx, int dtype, int ref_dtype, int ntime, int nlev, int nplev, long long ncol,
                                const double *plev, const void *ps, const void *ta_b, const void *ta_a, const void *hur_b,
                                const void *hur_a, const void *ua_b, const void *ua_a, const void *va_b, const void *va_a,
                                const void *tas_b, const void *tas_a, const void *hurs_b, const void *hurs_a,
                                const void *pshist_b, const void *pshist_a, double x_hi, double x_new, int ignore_top,
                                double *dta, double *dhur, double *dua, double *dva) {
    CHECK_COMMON(ctx, dtype, ntime, ncol);
    const bool ref = ref_dtype != 0;
    NEED(ctx, !ref || dtype == PGW_F32, "ref_dtype = 1 is the float32-file mode: dtype must be PGW_F32");
    NEED(ctx, ctx->nlev > 0 && nlev == ctx->nlev, "nlev must match pgw_set_levels");
    NEED(ctx, nplev >= 2 && nplev <= MAX_PLEV_WIDE, PLEV_RANGE_2);
    NEED(ctx, plev && ps && ta_b && hur_b && ua_b && va_b && tas_b && hurs_b && pshist_b, "null pointer");
    NEED(ctx, x_hi == 0.0 || (ta_a && hur_a && ua_a && va_a && tas_a && hurs_a && pshist_a), "record after the instant is NULL");
    NEED(ctx, dta && dhur && dua && dva, "output pointer is NULL");
    int rc = plev_table(ctx, nplev, plev);
    if (rc) return rc;
    if ((rc = status_reset(ctx))) return rc;
    const Levels lv = levels_of(ctx);
    const long long total = (long long)ntime * ncol;
    // O: 32-bit byte offsets while the largest array (a float64 output, or the records) stays below 4 GiB
    const unsigned long long big = (unsigned long long)ntime * ncol *
                                   std::max((unsigned long long)nlev * sizeof(double), (unsigned long long)nplev * elem_size(dtype));
    const bool o32 = !ctx->opt[PGW_OPT_FORCE_OFF64] && big < (1ull << 32);
    {
        Prof pr(ctx, PGW_K_DELTA_FIELDS);
        with_flow(dtype, ref, [&](auto t_, auto, auto ref_) {
            using T = decltype(t_);
            const PairSrc<T> dth = pair_src<T>(ta_b, ta_a, hur_b, hur_a, x_hi, x_new);
            const PairSrc<T> ds = pair_src<T>(tas_b, tas_a, hurs_b, hurs_a, x_hi, x_new);
            const DeltaSrc<T> ph = delta_src<T>(pshist_b, pshist_a, x_hi, x_new);
            const PairSrc<T> dwd = pair_src<T>(ua_b, ua_a, va_b, va_a, x_hi, x_new);
            with_offsets(o32, [&](auto o_) { with_int<2>(x_hi != 0.0, [&](auto lerp_) { with_plev(ctx, [&](const auto &pt) {
                // k_delta_quad<.., DELTAS = true>: blocks of 128, the quad kernel's dynamic LDS; no ERA fields, no e / QV outputs, no FusedFirst
                hipLaunchKernelGGL((k_delta_fields<T, decltype(o_), decltype(lerp_)::value != 0, decltype(ref_)::value, std::decay_t<decltype(pt)>>),
                                   dim3(nblocks(total, 128)), dim3(128), (size_t)(5 * nlev + 2) * sizeof(double), ctx->stream,
                                   pt, lv, ntime, ncol, (const T *)nullptr, (const T *)nullptr, (const T *)nullptr,
                                   (const T *)nullptr, (const T *)ps, dth, ds, ph, dwd, ignore_top ? 0 : 1, dta, (double *)nullptr,
                                   dhur, dua, dva, (double *)nullptr, 0, ctx->n_pure, ctx->d_status, 0.0,
                                   (const FusedFirst<T> *)nullptr);
            }); }); });
        });
    }
    HIPCHK(ctx, hipGetLastError());
    if ((rc = status_check(ctx))) return rc;
    return top_pressure_check(ctx, ignore_top);
}

extern "C" int pgw_reinterp_field(pgw_ctx *ctx, int dtype, int ntime, int nplev, long long ncol, const double *plev,
                                  const void *delta_b, const void *delta_a, double x_hi, double x_new, const void *dsfc_b,
                                  const void *dsfc_a, const void *pshist_b, const void *pshist_a, const void *era_field,
                                  const void *ps_era, const void *ps_pgw, int ignore_top, void *out) {
    CHECK_COMMON(ctx, dtype, ntime, ncol);
    NEED(ctx, nplev >= 2 && nplev <= MAX_PLEV_WIDE, PLEV_RANGE_2);
    NEED(ctx, plev && delta_b && era_field && ps_era && ps_pgw && out, "null pointer");
    NEED(ctx, (dsfc_b == nullptr) == (pshist_b == nullptr), "delta_sfc and ps_hist must be given together");
    NEED(ctx, ctx->nlev > 0, "pgw_set_levels has not been called");
    int rc = plev_table(ctx, nplev, plev);
    if (rc) return rc;
    if ((rc = status_reset(ctx))) return rc;
    Levels lv = levels_of(ctx);
    const long long total = (long long)ntime * ncol;
    {
        Prof pr(ctx, PGW_K_VERT_INTERP_DELTA);
        with_type(dtype, [&](auto t_) { with_int<2>(dsfc_b != nullptr, [&](auto sfc_) { with_plev(ctx, [&](const auto &pt) {
            using T = decltype(t_);
            hipLaunchKernelGGL((k_reinterp_field<T, decltype(sfc_)::value != 0, std::decay_t<decltype(pt)>>), dim3(nblocks(total, BLOCK)), dim3(BLOCK), 0,
                               ctx->stream, pt, lv, ntime, ncol, delta_src<T>(delta_b, delta_a, x_hi, x_new),
                               delta_src<T>(dsfc_b, dsfc_a, x_hi, x_new), delta_src<T>(pshist_b, pshist_a, x_hi, x_new),
                               (const T *)era_field, (const T *)ps_era, (const T *)ps_pgw, ignore_top ? 0 : 1, (T *)out,
                               ctx->d_status);
        }); }); });
    }
    HIPCHK(ctx, hipGetLastError());
    if ((rc = status_check(ctx))) return rc;
    return top_pressure_check(ctx, ignore_top);
}

// SFC: with the surface insertion; EVAP: the loop's ta + hur pair, which also leaves e (always with the surface insertion).
// Reference-dtype mode without EVAP is the ua + va pair after the loop: no surface form of it is instantiated.
template <typename T, typename TE0 = T, typename TE1 = T, typename TO = T, bool REF = false>
static void launch_reinterp_pair(pgw_ctx *ctx, const Levels &lv, int ntime, int nplev, long long ncol,
                                 const ReinterpPair<T, TE0, TE1, TO> &rv,
                                 const DeltaSrc<T> &p, const T *ps_era, const T *ps_pgw, bool sfc, int check_top) {
    // 32-bit byte offsets when every array (fields: nlev levels, delta records: nplev levels) is smaller than 4 GiB
    const unsigned long long big = (unsigned long long)ntime * (lv.nlev > nplev ? lv.nlev : nplev) * ncol * sizeof(TO);
    with_offsets(big < (1ull << 32) && !ctx->opt[PGW_OPT_FORCE_OFF64], [&](auto o_) { with_plev(ctx, [&](const auto &pt) {
        auto launch = [&](auto sfc_, auto evap_) {
            hipLaunchKernelGGL((k_reinterp_pair<T, decltype(sfc_)::value, decltype(o_), decltype(evap_)::value, TE0, TE1, TO, REF, std::decay_t<decltype(pt)>>),
                               dim3(nblocks((long long)ntime * ncol, BLOCK)), dim3(BLOCK), 2 * lv.nlev * sizeof(double), ctx->stream,
                               pt, lv, ntime, ncol, rv, p, ps_era, ps_pgw, check_top, ctx->d_status);
        };
        if (rv.evap) return launch(std::true_type(), std::true_type());
        if constexpr (!REF) { if (sfc) return launch(std::true_type(), std::false_type()); }
        launch(std::false_type(), std::false_type());
    }); });
}

extern "C" int pgw_reinterp_pair(pgw_ctx *ctx, int dtype, int ntime, int nplev, long long ncol, const double *plev,
                                 const void *const *delta_b, const void *const *delta_a, double x_hi, double x_new,
                                 const void *const *dsfc_b, const void *const *dsfc_a, const void *pshist_b,
                                 const void *pshist_a, const void *const *era_field, const void *ps_era, const void *ps_pgw,
                                 int ignore_top, void *const *out) {
    CHECK_COMMON(ctx, dtype, ntime, ncol);
    NEED(ctx, nplev >= 2 && nplev <= MAX_PLEV_WIDE, PLEV_RANGE_2);
    NEED(ctx, plev && delta_b && era_field && ps_era && ps_pgw && out, "null pointer");
    NEED(ctx, delta_b[0] && delta_b[1] && era_field[0] && era_field[1] && out[0] && out[1], "null pointer");
    NEED(ctx, (dsfc_b == nullptr) == (pshist_b == nullptr), "delta_sfc and ps_hist must be given together");
    NEED(ctx, !dsfc_b || (dsfc_b[0] && dsfc_b[1]), "null pointer");
    NEED(ctx, ctx->nlev > 0, "pgw_set_levels has not been called");
    const bool lerp = (x_hi != 0.0);
    NEED(ctx, !lerp || (delta_a && delta_a[0] && delta_a[1] && (!dsfc_b || (dsfc_a && dsfc_a[0] && dsfc_a[1] && pshist_a))),
         "the record after the instant is missing");
    int rc = plev_table(ctx, nplev, plev);
    if (rc) return rc;
    if ((rc = status_reset(ctx))) return rc;
    Levels lv = levels_of(ctx);
    {
        Prof pr(ctx, PGW_K_VERT_INTERP_DELTA);
        with_type(dtype, [&](auto t_) {
            using T = decltype(t_);
            ReinterpPair<T> rv;
            for (int v = 0; v < 2; ++v) {
                rv.d[v] = delta_src<T>(delta_b[v], lerp ? delta_a[v] : nullptr, x_hi, x_new);
                rv.sfc[v] = delta_src<T>(dsfc_b ? dsfc_b[v] : nullptr, (dsfc_b && lerp) ? dsfc_a[v] : nullptr, x_hi, x_new);
                rv.out[v] = (T *)out[v];
            }
            rv.era0 = (const T *)era_field[0]; rv.era1 = (const T *)era_field[1];
            rv.evap = nullptr;
            launch_reinterp_pair<T>(ctx, lv, ntime, nplev, ncol, rv, delta_src<T>(pshist_b, pshist_a, x_hi, x_new), (const T *)ps_era,
                                    (const T *)ps_pgw, dsfc_b != nullptr, ignore_top ? 0 : 1);
        });
    }
    HIPCHK(ctx, hipGetLastError());
    if ((rc = status_check(ctx))) return rc;
    return top_pressure_check(ctx, ignore_top);
}

// pressure levels that are ascending as given (no reversal, no logarithms): p, n and the extrema
static PlevTableWide ascending_plev_table(int nplev, const double *plev_asc) {
    PlevTableWide t;
    memset(&t, 0, sizeof(t));
    t.n = nplev; t.pmax = -INFINITY; t.pmin = INFINITY;
    for (int i = 0; i < nplev; ++i) {
        t.p[i] = plev_asc[i];
        if (t.p[i] > t.pmax) t.pmax = t.p[i];
        if (t.p[i] < t.pmin) t.pmin = t.p[i];
    }
    return t;
}

extern "C" int pgw_replace_delta_sfc(pgw_ctx *ctx, int dtype, int ntime, int nplev, long long ncol,
                                     const double *plev_asc, const void *delta, const void *delta_sfc,
                                     const void *ps_hist, void *out_P, void *out_delta) {
    CHECK_COMMON(ctx, dtype, ntime, ncol);
    NEED(ctx, nplev >= 1 && nplev <= MAX_PLEV_WIDE, PLEV_RANGE_1);
    NEED(ctx, plev_asc && delta && delta_sfc && ps_hist && out_P && out_delta, "null pointer");
    const PlevTableWide tw = ascending_plev_table(nplev, plev_asc);
    int rc = status_reset(ctx);
    if (rc) return rc;
    long long total = (long long)ntime * ncol;
    {
        Prof pr(ctx, PGW_K_VERT_INTERP_DELTA);
        with_type(dtype, [&](auto t_) { with_plev(tw, [&](const auto &pt) {
            using T = decltype(t_);
            hipLaunchKernelGGL((k_replace_delta_sfc<T, T, T, T, std::decay_t<decltype(pt)>>), dim3(nblocks(total, BLOCK)), dim3(BLOCK), 0, ctx->stream, pt, ntime, ncol,
                               (const T *)delta, (const T *)delta_sfc, (const T *)ps_hist, (T *)out_P, (T *)out_delta, ctx->d_status);
        }); });
    }
    HIPCHK(ctx, hipGetLastError());
    return status_check(ctx);
}

// ------------------------------------------------------------------ ps fixed-point loop
#ifndef PAIR_U
#define PAIR_U 4
#endif
#ifndef STEP_U
#define STEP_U 2      // measured 3 % faster than 4 for the pass kernel (finer stop above p_ref, fewer VGPRs)
#endif

static int launch_step(pgw_ctx *ctx, int dtype, int ntime, long long ncol, const void *ta, const void *evap,
                       const void *PS, const void *FIS, const double *phi_ref_era, const double *dphi_clim,
                       double *delta_ps, double *adj_ps, double p_ref, const double *p_ref_field,
                       double adj_factor, int full_column, int apply_adj = 1, DevStatus *st = nullptr,
                       DevStatus *clear = nullptr, bool ref = false) {
    if (!st) st = ctx->d_status;
    int vec = pick_vec(ctx, dtype, ncol, {ta, evap, PS, FIS, phi_ref_era, dphi_clim, delta_ps, adj_ps, p_ref_field}, 2);
    // fp64 state arrays are read with V doubles per lane: 16*V/2 B alignment follows from ncol % V == 0
    Levels lv = levels_of(ctx);
    Prof pr(ctx, PGW_K_ADJUST_PS_STEP);
    with_flow_vec(dtype, ref, vec, [&](auto t_, auto l_, auto ref_, auto v_) {
        using T = decltype(t_); using TL = decltype(l_);
        constexpr int V = decltype(v_)::value;
        hipLaunchKernelGGL((k_adjust_ps_step<T, TL, V, STEP_U, decltype(ref_)::value>), dim3(nblocks((long long)ntime * ncol / V, BLOCK)),
                           dim3(BLOCK), 0, ctx->stream, lv, ntime, ncol, (const TL *)ta, (const TL *)evap, (const T *)PS,
                           (const T *)FIS, phi_ref_era, dphi_clim, delta_ps, adj_ps, p_ref, p_ref_field, adj_factor, full_column,
                           apply_adj, st, clear);
    });
    return PGW_OK;
}

static int launch_phi_ref_hybrid(pgw_ctx *ctx, int dtype, int ntime, long long ncol, const void *ta, const void *hus,
                                 const void *PS, const void *FIS, double p_ref, double *phi_out, int full_column,
                                 const double *p_ref_field = nullptr, bool ref = false) {
    int vec = pick_vec(ctx, dtype, ncol, {ta, hus, PS, FIS, phi_out}, 2);
    Levels lv = levels_of(ctx);
    Prof pr(ctx, PGW_K_PHI_REF_HYBRID);
    with_flow_vec(dtype, ref, vec, [&](auto t_, auto, auto ref_, auto v_) {
        using T = decltype(t_);
        constexpr int V = decltype(v_)::value;
        hipLaunchKernelGGL((k_phi_ref_hybrid<T, V, STEP_U, decltype(ref_)::value>), dim3(nblocks((long long)ntime * ncol / V, BLOCK)),
                           dim3(BLOCK), 0, ctx->stream, lv, ntime, ncol, (const T *)ta, (const T *)hus, (const T *)PS, (const T *)FIS,
                           p_ref, p_ref_field, phi_out, full_column, ctx->d_status);
    });
    return PGW_OK;
}

static double max_err_of(pgw_ctx *ctx) {
    DevStatus *h = ctx->h_status;
    if (h->valid == 0) return NAN;              // xarray .max() of an all-NaN field
    double m;
    memcpy(&m, &h->max_bits, 8);
    return m;
}

#define QUAD_TPB 128      // 64 / 256 threads measured the same (2.16 / 2.17 / 2.17 ms same box)
#ifndef QUAD_U
#define QUAD_U 2          // levels per software-pipeline chunk of k_delta_quad
#endif

extern "C" int pgw_adjust_ps_step(pgw_ctx *ctx, int dtype, int ntime, long long ncol, const void *ta_pgw,
                                  const void *hur_pgw, const void *PS, const void *FIS, const double *phi_ref_era,
                                  const double *dphi_clim, double *delta_ps, double *adj_ps, double p_ref,
                                  const double *p_ref_field, double adj_factor, int apply_adj, double *max_abs_err) {
    CHECK_COMMON(ctx, dtype, ntime, ncol);
    NEED(ctx, ctx->nlev > 0, "pgw_set_levels has not been called");
    NEED(ctx, ta_pgw && hur_pgw && PS && FIS && phi_ref_era && dphi_clim && delta_ps && adj_ps, "null pointer");
    void *evap = nullptr;
    int rc = ws_get(ctx, 0, (size_t)ntime * ctx->nlev * ncol * elem_size(dtype), &evap);
    if (rc) return rc;
    rc = humidity_hybrid<2>(ctx, PGW_K_RH_TO_Q, dtype, ntime, ncol, hur_pgw, PS, ta_pgw, evap);
    if (rc) return rc;
    rc = status_reset(ctx);
    if (rc) return rc;
    launch_step(ctx, dtype, ntime, ncol, ta_pgw, evap, PS, FIS, phi_ref_era, dphi_clim, delta_ps, adj_ps, p_ref,
                p_ref_field, adj_factor, ctx->opt[PGW_OPT_FULL_COLUMN], apply_adj ? 1 : 0);
    HIPCHK(ctx, hipGetLastError());
    rc = status_check(ctx);
    if (max_abs_err) *max_abs_err = max_err_of(ctx);
    return rc;
}

static void launch_update_ps(pgw_ctx *ctx, int dtype, long long n, const void *PS, double *delta_ps, const double *adj_ps,
                             void *ps_pgw) {
    with_type(dtype, [&](auto t_) {
        using T = decltype(t_);
        hipLaunchKernelGGL((k_update_ps<T>), dim3(nblocks(n, BLOCK)), dim3(BLOCK), 0, ctx->stream, n, (const T *)PS, delta_ps, adj_ps,
                           (T *)ps_pgw);
    });
}

extern "C" int pgw_reinterp_pass(pgw_ctx *ctx, int dtype, int ntime, int nplev, long long ncol, const double *plev,
                                 const void *const *delta_b, const void *const *delta_a, double x_hi, double x_new,
                                 const void *const *dsfc_b, const void *const *dsfc_a, const void *pshist_b,
                                 const void *pshist_a, const void *T_era, const void *RELHUM_era, const void *PS,
                                 const void *FIS, const double *phi_ref_era, const double *dphi_clim, double *delta_ps,
                                 double *adj_ps, double p_ref, double adj_factor, int ignore_top, void *ps_pgw,
                                 void *ta_pgw, void *hur_pgw, double *max_abs_err) {
    CHECK_COMMON(ctx, dtype, ntime, ncol);
    NEED(ctx, nplev >= 2 && nplev <= MAX_PLEV_WIDE, PLEV_RANGE_2);
    NEED(ctx, ctx->nlev > 0, "pgw_set_levels has not been called");
    NEED(ctx, plev && delta_b && dsfc_b && pshist_b && T_era && RELHUM_era && PS && FIS && phi_ref_era && dphi_clim && delta_ps &&
         adj_ps && ps_pgw && ta_pgw && hur_pgw, "null pointer");
    NEED(ctx, delta_b[0] && delta_b[1] && dsfc_b[0] && dsfc_b[1], "null pointer");
    const bool lerp = (x_hi != 0.0);
    NEED(ctx, !lerp || (delta_a && delta_a[0] && delta_a[1] && dsfc_a && dsfc_a[0] && dsfc_a[1] && pshist_a),
         "the record after the instant is missing");
    void *evap = nullptr;
    int rc = ws_get(ctx, 0, (size_t)ntime * ctx->nlev * ncol * elem_size(dtype), &evap);
    if (rc) return rc;
    if ((rc = plev_table(ctx, nplev, plev))) return rc;
    if ((rc = status_reset(ctx))) return rc;
    Levels lv = levels_of(ctx);
    const long long n2 = (long long)ntime * ncol;
    launch_update_ps(ctx, dtype, n2, PS, delta_ps, adj_ps, ps_pgw);      // step_03:192-193
    {   // :202-216 for ta and hur, + e of functions.py:123
        Prof pr(ctx, PGW_K_VERT_INTERP_DELTA);
        with_type(dtype, [&](auto t_) {
            using T = decltype(t_);
            ReinterpPair<T> rv;
            for (int v = 0; v < 2; ++v) {
                rv.d[v] = delta_src<T>(delta_b[v], lerp ? delta_a[v] : nullptr, x_hi, x_new);
                rv.sfc[v] = delta_src<T>(dsfc_b[v], lerp ? dsfc_a[v] : nullptr, x_hi, x_new);
            }
            rv.era0 = (const T *)T_era; rv.era1 = (const T *)RELHUM_era;
            rv.out[0] = (T *)ta_pgw; rv.out[1] = (T *)hur_pgw;
            rv.evap = (T *)evap;
            launch_reinterp_pair<T>(ctx, lv, ntime, nplev, ncol, rv, delta_src<T>(pshist_b, pshist_a, x_hi, x_new), (const T *)PS,
                                    (const T *)ps_pgw, true, ignore_top ? 0 : 1);
        });
    }
    // :262-308: the pass on the re-interpolated fields (delta_ps already carries this pass's increment)
    launch_step(ctx, dtype, ntime, ncol, ta_pgw, evap, PS, FIS, phi_ref_era, dphi_clim, delta_ps, adj_ps, p_ref, nullptr,
                adj_factor, ctx->opt[PGW_OPT_FULL_COLUMN], 0);
    HIPCHK(ctx, hipGetLastError());
    rc = status_check(ctx);
    if (max_abs_err) *max_abs_err = max_err_of(ctx);
    if (rc) return rc;
    return top_pressure_check(ctx, ignore_top);
}

extern "C" int pgw_update_ps(pgw_ctx *ctx, int dtype, long long n, const void *PS, double *delta_ps,
                             const double *adj_ps, void *ps_pgw) {
    NEED(ctx, dtype == PGW_F32 || dtype == PGW_F64, "dtype must be PGW_F32 or PGW_F64");
    NEED(ctx, n >= 1 && PS && delta_ps && adj_ps && ps_pgw, "bad argument");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    launch_update_ps(ctx, dtype, n, PS, delta_ps, adj_ps, ps_pgw);
    HIPCHK(ctx, hipGetLastError());
    return PGW_OK;
}

extern "C" int pgw_phi_ref_hybrid(pgw_ctx *ctx, int dtype, int ntime, long long ncol, const void *T, const void *QV,
                                  const void *PS, const void *FIS, double p_ref, const double *p_ref_field,
                                  double *phi_ref) {
    CHECK_COMMON(ctx, dtype, ntime, ncol);
    NEED(ctx, ctx->nlev > 0, "pgw_set_levels has not been called");
    NEED(ctx, T && QV && PS && FIS && phi_ref, "null pointer");
    int rc = status_reset(ctx);
    if (rc) return rc;
    launch_phi_ref_hybrid(ctx, dtype, ntime, ncol, T, QV, PS, FIS, p_ref, phi_ref, ctx->opt[PGW_OPT_FULL_COLUMN], p_ref_field);
    HIPCHK(ctx, hipGetLastError());
    return status_check(ctx);
}

// ---- latitude-band sharding (pgw_set_reduce_hook).  One vector per loop launch: BandVector of pgw_loop_control.h.
static int call_reduce(pgw_ctx *ctx, BandVector &v, int np) {
    ctx->band_reduces += 1;
    if (ctx->reduce_fn(v.v, BandVector::length(np), ctx->reduce_user) != 0) {
        ctx->band_agreed = true;                    // the exchange itself is broken: nobody is met by sending more
        ctx->err = "the reduce hook (pgw_set_reduce_hook) failed";
        ctx->err_col = -1;
        return PGW_ERR_REDUCE;
    }
    return PGW_OK;
}

// An error of THIS band only (a data error found before the loop's first launch, a failed allocation, a HIP error - at
// any point of the file): the other bands are waiting, or about to wait, in their next reduce.  Meet them there with the
// status - in the slot of the kernels before the loop while no reduce has been made, in the first pass's status slot of a
// continuation launch afterwards - so every rank returns it instead of blocking until the backend's timeout.
static int band_fail(pgw_ctx *ctx, int code, int max_n_iter) {
    if (!ctx->reduce_fn || code == PGW_OK || ctx->band_agreed) return code;
    const std::string text = ctx->err;
    const long long col = ctx->err_col;
    const bool first = ctx->band_reduces == 0;
    const int np = first ? launch_passes(true, ctx->opt[PGW_OPT_LOOP_GUESS], max_n_iter, max_n_iter) : std::max(ctx->band_next_np, 1);
    BandVector v;
    v.blank(np);
    if (first) v.set_pre(code); else v.set(0, code, false, -INFINITY);
    call_reduce(ctx, v, np);
    ctx->band_agreed = true;
    ctx->err = text;
    ctx->err_col = col;
    return code;
}

extern "C" int pgw_band_abort(pgw_ctx *ctx, int code, int max_n_iter) {
    if (!ctx) return PGW_ERR_ARG;
    ctx->band_reduces = 0; ctx->band_next_np = 0; ctx->band_agreed = false;
    band_fail(ctx, code == PGW_OK ? PGW_ERR_ARG : code, max_n_iter);
    return PGW_OK;
}

extern "C" int pgw_set_reduce_hook(pgw_ctx *ctx, pgw_reduce_max_fn fn, void *user) {
    if (!ctx) return PGW_ERR_ARG;
    ctx->reduce_fn = fn;
    ctx->reduce_user = fn ? user : nullptr;
    return PGW_OK;
}

// State of the loop in workspace slot 1, six arrays of n2 doubles: phi_ref_era | dphi_clim | delta_ps | adj_ps | p_ref per
// column (local p_ref) | its level index (n2 ints) and, in the other half of the sixth array, the flags of
// k_delta_quad's FusedFirst (one byte per 64 columns).
struct LoopState { double *phi_era, *dphi, *delta_ps, *adj_ps, *pref_f; int *pref_idx; unsigned char *era_flags; };
static int loop_state(pgw_ctx *ctx, long long n2, LoopState *ls) {
    void *state = nullptr;
    int rc;
    if ((rc = ws_get(ctx, 1, (size_t)n2 * 6 * sizeof(double), &state))) return rc;
    ls->phi_era = (double *)state; ls->dphi = ls->phi_era + n2; ls->delta_ps = ls->dphi + n2; ls->adj_ps = ls->delta_ps + n2;
    ls->pref_f = ls->adj_ps + n2;
    ls->pref_idx = (int *)(ls->pref_f + n2);
    ls->era_flags = (unsigned char *)(ls->pref_idx + n2);          // n2 / 64 + 1 <= 4 * n2 bytes
    return PGW_OK;
}

// plev coordinate in file order for the local reference level (p_ref_inp = None); nplev = 0: fixed p_ref, an empty table
static PlevTable file_order_table(int nplev, const double *plev_file) {
    PlevTable t;
    memset(&t, 0, sizeof(t));
    t.n = nplev;
    for (int i = 0; i < nplev; ++i) t.p[i] = plev_file[i];
    return t;
}

// n blank blocks in the pinned host area behind the read-back blocks: what a copy arms per-pass device blocks with
static DevStatus *blank_blocks(pgw_ctx *ctx, int n) {
    DevStatus *blank = ctx->h_status + 2 + MULTI_MAX_PASS;
    for (int k = 0; k < n; ++k) blank[k] = blank_status();
    return blank;
}

// g * (time-interpolated zg delta at p_ref)   step_03:292-295;   + delta_ps = adj_ps = 0   :182-184
static void launch_dphi_clim(pgw_ctx *ctx, int dtype, bool ref, long long n2, const void *zg_b, const void *zg_a, double x_hi,
                             double x_new, const LoopState &ls) {
    with_flow(dtype, ref, [&](auto t_, auto, auto ref_) {
        using T = decltype(t_);
        hipLaunchKernelGGL((k_dphi_clim<T, decltype(ref_)::value>), dim3(nblocks(n2, BLOCK)), dim3(BLOCK), 0, ctx->stream, n2,
                           delta_src<T>(zg_b, zg_a, x_hi, x_new), CON_G, ls.dphi, ls.delta_ps, ls.adj_ps);
    });
}

// delta_ps += adj_ps; the column's reference level (never lower than the last pass's); g * zg there   :192, 219-253, 292-295
static void launch_local_p_ref(pgw_ctx *ctx, int dtype, bool ref, const PlevTable &ptf, long long n2, long long ncol, const void *PS,
                               const void *zg3_b, const void *zg3_a, double x_hi, double x_new, int first_pass, const LoopState &ls) {
    with_flow(dtype, ref, [&](auto t_, auto, auto ref_) {
        using T = decltype(t_);
        hipLaunchKernelGGL((k_local_p_ref<T, decltype(ref_)::value>), dim3(nblocks(n2, BLOCK)), dim3(BLOCK), 0, ctx->stream, ptf,
                           ctx->h_akN, ctx->h_bkN, n2, (const T *)PS, ls.delta_ps, ls.adj_ps, delta_src<T>(zg3_b, zg3_a, x_hi, x_new),
                           ncol, first_pass, ls.pref_f, ls.pref_idx, ls.dphi, ctx->d_status);
    });
}

// ps_pgw = PS + dps and hus_pgw from e on the final levels (:262-266, 370); the first qv_done_levels levels of hus_pgw are
// already written, and with `marks` so are each column's levels from its mark on (by the converged loop pass)
static void launch_finalize(pgw_ctx *ctx, int dtype, bool ref, int ntime, long long ncol, const void *PS, const double *dps,
                            const void *evap, void *ps_pgw, void *hus_pgw, int qv_done_levels,
                            const unsigned short *marks = nullptr) {
    int vec = pick_vec(ctx, dtype, ncol, {PS, evap, ps_pgw, hus_pgw, dps});
    Levels lv = levels_of(ctx);
    Prof pr(ctx, PGW_K_FINALIZE);
    with_flow_vec(dtype, ref, vec, [&](auto t_, auto l_, auto ref_, auto v_) {
        using T = decltype(t_); using TL = decltype(l_);
        constexpr int V = decltype(v_)::value;
        hipLaunchKernelGGL((k_finalize_ps_hus<T, TL, V, decltype(ref_)::value>), dim3(nblocks((long long)ntime * ncol / V, BLOCK)),
                           dim3(BLOCK), 0, ctx->stream, lv, ntime, ncol, (const T *)PS, dps, (const TL *)evap, (T *)ps_pgw,
                           (TL *)hus_pgw, qv_done_levels, marks);
    });
}

// The loop of step_03_apply_to_era.py:182-319 given the iterate-independent vapour pressure
// `evap` = hur_pgw/100 * e_sat(ta_pgw) (functions.py:123).  Shared by pgw_adjust_ps_loop and
// pgw_step03_file.  The host reads max|err| after every pass (status copy + stream synchronisation) before it
// launches the next - the reference's control flow literally (four device-assisted variants, with the passes
// enqueued ahead of the host, all measured slower: DESIGN.md section 4, "tried and dropped").
struct PsLoopArgs {
    int dtype = PGW_F64, ntime = 0;
    long long ncol = 0;
    const void *PS = nullptr, *FIS = nullptr, *T = nullptr, *QV = nullptr;     // ERA state
    const void *ta_pgw = nullptr, *evap = nullptr;                             // PGW levels
    // zg delta records bracketing the instant: at p_ref (ntime, ncol), or with local_nplev > 0 the full (ntime, nplev, ncol)
    const void *dzg_b = nullptr, *dzg_a = nullptr;
    double x_hi = 0.0, x_new = 0.0;
    double p_ref = 0.0, adj_factor = 0.0;
    LoopControl ctl{0.0, 0};                                                   // thresh, max_n_iter, where max |err| per pass goes
    void *ps_pgw = nullptr, *hus_pgw = nullptr;                                // outputs (may be null)
    int *n_iter = nullptr;
    // local_nplev > 0 selects p_ref_inp = None (step_03:219-253); `plev_file` is then the plev coordinate in file order
    int local_nplev = 0;
    const double *plev_file = nullptr;
    // pgw_step03_file with the model-top check off: nothing is read back before the first pass; the status block keeps the
    // first error any kernel reported, in stream order, so the first pass's check raises what an immediate check would have
    bool status_armed = false;
    int qv_done_levels = 0;          // leading levels of hus_pgw the caller has already written
    bool ref = false;                // reference-dtype mode
    // pgw_step03_file, PGW_OPT_FUSED_FIRST: k_delta_quad has run the ERA-state scan and pass 1 for the groups of columns it
    // did not flag - the loop state in workspace slot 1, dps_hist[0] and the status block of pass 1 hold their results.  The
    // first launch is then two: pass 1 for the flagged groups alone (k_ps_loop_multi<.., FLAGGED>), and passes 2 .. np for
    // all columns as a continuation launch.
    bool fused_first = false;
    // PGW_OPT_QV_FROM_PASS may apply.  pgw_step03_file with PGW_OPT_QUAD = 0 says no: the pair kernels are kept as an independent
    // cross-check of the production path, and so is the QV their files get - all of it from the finalize kernel's division
    bool qv_from_pass = true;
    // PGW_OPT_FINISH_IN_PASS, pgw_step03_file: the launch of the surface riders, which depend on nothing else in the file.
    // The multi-pass loop enqueues it behind its first launch's status read-back, where the stream would otherwise stand
    // idle until the host has decided; empty: the caller has launched them
    std::function<int()> riders;
};

// The loop has stopped: the pass count goes to the caller; out of passes is the reference's error (:315-319).
static int loop_end(pgw_ctx *ctx, const LoopControl &lc, LoopControl::Verdict verdict, int *n_iter) {
    if (n_iter) *n_iter = lc.n_iter();
    return verdict == LoopControl::NOT_CONVERGED ? fail_status(ctx, PGW_ERR_NOT_CONVERGED) : PGW_OK;
}

// Loop control of a whole-file call: its results go to the argument struct, the history NaN where no pass is recorded.
static LoopControl file_loop_control(pgw_file_args *a) {
    const int hist_len = (int)(sizeof(a->max_err_hist) / sizeof(a->max_err_hist[0]));
    a->n_iter = 0;
    for (int i = 0; i < hist_len; ++i) a->max_err_hist[i] = NAN;
    return LoopControl{a->thresh, a->max_n_iter, 1, a->max_err_hist, hist_len};
}

// ---- several passes per launch (k_ps_loop_multi): fixed or local p_ref, wave-level early exit.  phi_ref of the ERA state,
// g * dzg and the zeroed state are produced by the first launch; LoopControl is applied to the recorded maxima.
static int ps_loop_multi(pgw_ctx *ctx, const PsLoopArgs &a, const LoopState &ls) {
    const int dtype = a.dtype, ntime = a.ntime;
    const long long ncol = a.ncol, n2 = (long long)ntime * ncol;
    const bool local = a.local_nplev > 0;
    const PlevTable ptf = file_order_table(a.local_nplev, a.plev_file);
    int rc;
    void *histv = nullptr;
    if ((rc = ws_get(ctx, 6, (size_t)n2 * MULTI_MAX_PASS * sizeof(double), &histv))) return rc;
    double *dps_hist = (double *)histv;
    DevStatus *mst = ctx->d_status + 2;                                // device per-pass blocks
    DevStatus *hback = ctx->h_status + 1;                              // [0] = block 0 (ERA-state scan / earlier kernels), [1..] passes
    DevStatus *hzero = blank_blocks(ctx, MULTI_MAX_PASS);
    // PGW_OPT_QV_FROM_PASS: the last pass of every launch of the FLAGGED = false, fixed-p_ref kernel stores the QV it
    // forms below p_ref into hus_pgw and marks how far each column got.  When that pass turns out to be the converged one
    // (the host predicts it: loop_guess), the finalize kernel has only the levels above the marks left; otherwise it
    // runs over all of them as before and overwrites what was speculated.  hus_pgw must not be an array the loop reads.
    unsigned short *marks = nullptr;
    if (ctx->opt[PGW_OPT_QV_FROM_PASS] && a.qv_from_pass && !local && a.hus_pgw && a.hus_pgw != a.QV && a.hus_pgw != a.T && a.hus_pgw != a.ta_pgw &&
        a.hus_pgw != a.evap) {
        void *m = nullptr;
        if ((rc = ws_get(ctx, 4, (size_t)n2 * sizeof(unsigned short), &m))) return rc;
        marks = (unsigned short *)m;
    }
    // PGW_OPT_FINISH_IN_PASS: the storing pass also walks its columns' remaining hybrid levels and writes ps_pgw
    const bool finish = marks && ctx->opt[PGW_OPT_FINISH_IN_PASS] && a.ps_pgw && a.ps_pgw != a.PS;
    StoredPass sp;                 // the pass that stored QV in the launch just read back, and what the stopping rule made of it
    ctx->last_qv_from_pass = false; ctx->last_qv_skipped = 0;
    if (!a.status_armed && (rc = status_reset(ctx))) return rc;
    LoopControl lc = a.ctl;
    LoopControl::Verdict verdict = LoopControl::CONTINUE;
    bool first = true;
    unsigned long long touched = 0;
    const double *conv = nullptr;  // delta_ps the converged pass used
    int launched = 0;
    while (verdict == LoopControl::CONTINUE) {
        const int np = launch_passes(first, ctx->opt[PGW_OPT_LOOP_GUESS], lc.max_n_iter, lc.allowed());
        ctx->band_next_np = np;
        if (first && ctx->opt[PGW_OPT_TEST_FAIL] == 2) return fail(ctx, PGW_ERR_HIP, "PGW_OPT_TEST_FAIL = 2: forced failure before the first loop launch");
        if (!first && ctx->opt[PGW_OPT_TEST_FAIL] == 3) return fail(ctx, PGW_ERR_HIP, "PGW_OPT_TEST_FAIL = 3: forced failure before a continuation launch");
        const bool fused_launch = first && a.fused_first;              // (block of pass 1: armed before the delta kernel)
        if (!fused_launch) HIPCHK(ctx, hipMemcpyAsync(mst, hzero, sizeof(DevStatus) * np, hipMemcpyHostToDevice, ctx->stream));
        else if (np > 1) HIPCHK(ctx, hipMemcpyAsync(mst + 1, hzero + 1, sizeof(DevStatus) * (np - 1), hipMemcpyHostToDevice, ctx->stream));
        {
            // one column per lane (two columns: 168 VGPRs + scratch; measured 1.36 vs 1.39 ms before the log table)
            constexpr int MULTI_MAXV = 1;
            int vec = pick_vec(ctx, dtype, ncol, {a.ta_pgw, a.evap, a.T, a.QV, a.PS, a.FIS, ls.phi_era, ls.dphi, ls.delta_ps, ls.adj_ps, dps_hist,
                                                   marks ? a.hus_pgw : nullptr /* the storing pass writes V-wide rows */,
                                                   finish ? a.ps_pgw : nullptr}, MULTI_MAXV);
            Levels lv = levels_of(ctx);
            Prof pr(ctx, PGW_K_PS_LOOP_MULTI);
            const LocalPRef loc{ptf, ctx->h_akN, ctx->h_bkN, ls.pref_f, ls.pref_idx};
            with_flow_vec(dtype, a.ref, vec, [&](auto t_, auto l_, auto ref_, auto v_) {
                using T = decltype(t_); using TL = decltype(l_);
                constexpr int V = decltype(v_)::value;
                // `n` passes from the state as it stands (init: from the ERA state) into `blocks` and the rows of `hist`
                constexpr bool qv_pass = QV_FROM_PASS<TL, decltype(ref_)::value>;
                const bool finish_pass = finish && FINISH_IN_PASS<TL, decltype(ref_)::value>;
                int stored_k = -1;
                auto launch = [&](auto local_, auto flagged_, double p_ref, int init, int n, DevStatus *blocks, double *hist,
                                  unsigned char *flags, DevStatus *st_era) {
                    const bool store = qv_pass && marks && !decltype(local_)::value && !decltype(flagged_)::value;
                    if (store) stored_k = (int)(blocks - mst) + n - 1;
                    hipLaunchKernelGGL((k_ps_loop_multi<T, TL, V, STEP_U, decltype(ref_)::value, decltype(local_)::value, decltype(flagged_)::value>),
                                       dim3(nblocks(n2 / V, BLOCK)), dim3(BLOCK), 0, ctx->stream, lv, ntime, ncol, (const T *)a.T,
                                       (const T *)a.QV, (const TL *)a.ta_pgw, (const TL *)a.evap, (const T *)a.PS, (const T *)a.FIS,
                                       delta_src<T>(a.dzg_b, a.dzg_a, a.x_hi, a.x_new), ls.phi_era, ls.dphi, ls.delta_ps, ls.adj_ps,
                                       hist, p_ref, a.adj_factor, init, n, ctx->d_status, blocks, loc, flags, st_era,
                                       store ? (TL *)a.hus_pgw : nullptr, a.qv_done_levels, marks,
                                       store && finish_pass ? (T *)a.ps_pgw : nullptr);
                };
                constexpr std::true_type yes{};
                constexpr std::false_type no{};
                if (fused_launch) {
                    launch(no, yes, a.p_ref, 1, 1, mst, dps_hist, ls.era_flags, ctx->d_status + 1);
                    if (np > 1) launch(no, no, a.p_ref, 0, np - 1, mst + 1, dps_hist + n2, nullptr, nullptr);
                } else if (!local)
                    launch(no, no, a.p_ref, first ? 1 : 0, np, mst, dps_hist, nullptr, nullptr);
                else if constexpr (V == 1)                                 // MULTI_MAXV = 1: always this branch
                    launch(yes, no, 0.0, first ? 1 : 0, np, mst, dps_hist, nullptr, nullptr);
                sp.launched(stored_k, finish_pass);
            });
        }
        HIPCHK(ctx, hipGetLastError());
        launched += np;
        HIPCHK(ctx, hipMemcpyAsync(hback, ctx->d_status, sizeof(DevStatus), hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(ctx, hipMemcpyAsync(hback + 1, mst, sizeof(DevStatus) * np, hipMemcpyDeviceToHost, ctx->stream));
        if (first && a.riders) {
            // the host waits for the copies only; the riders run while it reads the figures, and whatever it enqueues next -
            // a continuation launch, the finalize kernel, the next file - queues behind them
            HIPCHK(ctx, hipEventRecord(ctx->status_read, ctx->stream));
            if ((rc = a.riders())) return rc;
            HIPCHK(ctx, hipEventSynchronize(ctx->status_read));
        } else
            HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
        // figures of this launch; with a reduce hook: their maxima over the bands of the file
        BandVector red;
        red.set_pre(first ? hback[0].code : 0);
        for (int k = 0; k < np; ++k) {
            const DevStatus &h = hback[1 + k];
            double e = -INFINITY;
            if (h.valid) memcpy(&e, &h.max_bits, 8);
            red.set(k, h.code, h.valid != 0, e);
        }
        if (ctx->reduce_fn && (rc = call_reduce(ctx, red, np))) return rc;
        if (first && red.pre() != 0) {                                 // earlier kernels of the file / the ERA-state scan
            ctx->band_agreed = true;                                   // every band has this status now
            if (hback[0].code == 0) return fail_status(ctx, red.pre());        // another band's status
            *ctx->h_status = hback[0];
            return fail_status(ctx, hback[0].code, (long long)hback[0].col);
        }
        for (int k = 0; k < np && verdict == LoopControl::CONTINUE; ++k) {
            const DevStatus &h = hback[1 + k];
            if (red.code(k) != 0) {
                ctx->band_agreed = true;
                return h.code != 0 ? fail_status(ctx, h.code, (long long)h.col) : fail_status(ctx, red.code(k));
            }
            touched += h.levels_touched;
            verdict = lc.record(red.err(k));
            if (verdict == LoopControl::CONVERGED) {
                conv = dps_hist + (size_t)k * n2;
                sp.decided(verdict, k, red.err(k));
                // hus_pgw holds this pass's QV from the marks on
                if (sp.final_step() != StoredPass::ALL_LEVELS) ctx->last_qv_skipped = h.qv_stored;
            }
        }
        first = false;
    }
    // every band leaves the loop here, on figures all of them have: nobody waits in a reduce of this file any more
    ctx->band_agreed = true;
    ctx->last_passes_launched = launched;
    if ((rc = loop_end(ctx, lc, verdict, a.n_iter))) return rc;
    ctx->opt[PGW_OPT_LOOP_GUESS] = std::min(std::max(lc.n_iter(), 1), MULTI_MAX_PASS);
    ctx->last_levels_touched = touched;
    const StoredPass::Final fin = sp.final_step();
    ctx->last_qv_from_pass = fin != StoredPass::ALL_LEVELS;
    if ((a.ps_pgw || a.hus_pgw) && fin != StoredPass::NOTHING)
        launch_finalize(ctx, dtype, a.ref, ntime, ncol, a.PS, conv, a.evap, a.ps_pgw, a.hus_pgw, a.qv_done_levels,
                        fin == StoredPass::ABOVE_MARKS ? marks : nullptr);
    HIPCHK(ctx, hipGetLastError());
    return PGW_OK;
}

// ---- one pass per launch (PGW_OPT_MULTIPASS = 0, or the full-column option: a per-pass traffic probe)
static int ps_loop_single(pgw_ctx *ctx, const PsLoopArgs &a, const LoopState &ls) {
    const int dtype = a.dtype, ntime = a.ntime, full_column = ctx->opt[PGW_OPT_FULL_COLUMN];
    const long long ncol = a.ncol, n2 = (long long)ntime * ncol;
    const bool local = a.local_nplev > 0;
    const PlevTable ptf = file_order_table(a.local_nplev, a.plev_file);
    int rc;
    if (local) {
        HIPCHK(ctx, hipMemsetAsync(ls.delta_ps, 0, sizeof(double) * 2 * n2, ctx->stream));    // :182-184
    } else {
        // phi_ref_era: constant over the iterations for a fixed p_ref (step_03:280-287 recomputes it).
        if (!a.status_armed && (rc = status_reset(ctx))) return rc;
        launch_phi_ref_hybrid(ctx, dtype, ntime, ncol, a.T, a.QV, a.PS, a.FIS, a.p_ref, ls.phi_era, full_column, nullptr, a.ref);
        HIPCHK(ctx, hipGetLastError());
        if (!a.status_armed && (rc = status_check(ctx))) return rc;
        launch_dphi_clim(ctx, dtype, a.ref, n2, a.dzg_b, a.dzg_a, a.x_hi, a.x_new, ls);
    }
    ctx->last_qv_from_pass = false; ctx->last_qv_skipped = 0;

    LoopControl lc = a.ctl;
    // :186, 189: the reference enters the loop on inf > thresh (no pass at all for a threshold of inf or NaN)
    LoopControl::Verdict verdict = INFINITY > lc.thresh ? LoopControl::CONTINUE : LoopControl::CONVERGED;
    unsigned long long touched = 0;
    // Fixed p_ref: the passes alternate between the two status blocks and each pass clears the other one for its
    // successor, so no reset copy is enqueued per pass (the read-back of the block being cleared was enqueued
    // before this pass was launched).
    DevStatus *blk[2] = {ctx->d_status, ctx->d_status + 1};
    while (verdict == LoopControl::CONTINUE) {
        const int done = lc.n_iter();                                      // passes before this one
        const bool reset_here = local || done == 0;
        if (reset_here && !(a.status_armed && done == 0) && (rc = status_reset(ctx))) return rc;
        DevStatus *cur = local ? ctx->d_status : blk[done & 1];
        if (local) {
            launch_local_p_ref(ctx, dtype, a.ref, ptf, n2, ncol, a.PS, a.dzg_b, a.dzg_a, a.x_hi, a.x_new, done == 0 ? 1 : 0, ls);
            launch_phi_ref_hybrid(ctx, dtype, ntime, ncol, a.T, a.QV, a.PS, a.FIS, 0.0, ls.phi_era, full_column, ls.pref_f, a.ref);   // :280-287
            launch_step(ctx, dtype, ntime, ncol, a.ta_pgw, a.evap, a.PS, a.FIS, ls.phi_era, ls.dphi, ls.delta_ps, ls.adj_ps, 0.0,
                        ls.pref_f, a.adj_factor, full_column, 0, nullptr, nullptr, a.ref);
        } else {
            launch_step(ctx, dtype, ntime, ncol, a.ta_pgw, a.evap, a.PS, a.FIS, ls.phi_era, ls.dphi, ls.delta_ps, ls.adj_ps, a.p_ref,
                        nullptr, a.adj_factor, full_column, 1, cur, blk[(done + 1) & 1], a.ref);
        }
        HIPCHK(ctx, hipGetLastError());
        if ((rc = status_check(ctx, cur))) return rc;
        touched += ctx->h_status->levels_touched;
        verdict = lc.record(max_err_of(ctx));                              // :308-319
    }
    if ((rc = loop_end(ctx, lc, verdict, a.n_iter))) return rc;
    ctx->last_levels_touched = touched;
    if (a.ps_pgw || a.hus_pgw)
        launch_finalize(ctx, dtype, a.ref, ntime, ncol, a.PS, ls.delta_ps, a.evap, a.ps_pgw, a.hus_pgw, a.qv_done_levels);
    HIPCHK(ctx, hipGetLastError());
    return PGW_OK;
}

static int run_ps_loop(pgw_ctx *ctx, const PsLoopArgs &a) {
    if (ctx->opt[PGW_OPT_TEST_FAIL] == 1) return fail(ctx, PGW_ERR_HIP, "PGW_OPT_TEST_FAIL = 1: forced workspace failure (ws_get)");
    LoopState ls;
    int rc;
    if ((rc = loop_state(ctx, (long long)a.ntime * a.ncol, &ls))) return rc;
    const bool multipass = ctx->opt[PGW_OPT_MULTIPASS] && !ctx->opt[PGW_OPT_FULL_COLUMN];
    NEED(ctx, !ctx->reduce_fn || multipass, "a reduce hook (latitude-band sharding) needs the multi-pass loop: "
                                            "PGW_OPT_MULTIPASS = 1, PGW_OPT_FULL_COLUMN = 0");
    return multipass ? ps_loop_multi(ctx, a, ls) : ps_loop_single(ctx, a, ls);
}

extern "C" int pgw_adjust_ps_loop(pgw_ctx *ctx, int dtype, int ntime, long long ncol, const void *PS,
                                  const void *FIS, const void *T, const void *QV, const void *ta_pgw,
                                  const void *hur_pgw, const void *dzg_pref, double p_ref, double adj_factor,
                                  double thresh, int max_n_iter, void *ps_pgw, void *hus_pgw, int *n_iter,
                                  double *max_err_hist) {
    CHECK_COMMON(ctx, dtype, ntime, ncol);
    NEED(ctx, ctx->nlev > 0, "pgw_set_levels has not been called");
    NEED(ctx, PS && FIS && T && QV && ta_pgw && hur_pgw && dzg_pref, "null pointer");
    void *evap = nullptr;
    int rc;
    if ((rc = ws_get(ctx, 0, (size_t)ntime * ctx->nlev * ncol * elem_size(dtype), &evap))) return rc;
    // e = hur_pgw/100 * e_sat(ta_pgw): iterate-independent part of :262-266
    if ((rc = humidity_hybrid<2>(ctx, PGW_K_RH_TO_Q, dtype, ntime, ncol, hur_pgw, PS, ta_pgw, evap))) return rc;
    PsLoopArgs la;
    la.dtype = dtype; la.ntime = ntime; la.ncol = ncol;
    la.PS = PS; la.FIS = FIS; la.T = T; la.QV = QV;
    la.ta_pgw = ta_pgw; la.evap = evap;
    la.dzg_b = dzg_pref;                                  // the delta at the instant: no bracket
    la.p_ref = p_ref; la.adj_factor = adj_factor;
    la.ps_pgw = ps_pgw; la.hus_pgw = hus_pgw;
    la.n_iter = n_iter; la.ctl = LoopControl{thresh, max_n_iter, 1, max_err_hist, max_n_iter};
    return run_ps_loop(ctx, la);
}

// ------------------------------------------------------------------ whole file, settings.i_reinterp = 1
// step_03_apply_to_era.py:182-343 with i_reinterp = 1: in every pass the ERA ta / hur fields and their deltas are
// interpolated onto the CURRENT model-level pressures (:202-216), ua / va once after convergence (:330-343).  Fixed or local
// reference level (p_ref_inp = None, :219-253), float64 / float32 storage, reference-dtype mode on float32 files.  One launch
// sequence and one host read-back (max |err|, status) per pass - the loop control is the reference's.
static int run_reinterp_file(pgw_ctx *ctx, pgw_file_args *a, int check_top) {
    const int dtype = a->dtype, ntime = a->ntime, N = a->nlev, S = a->nplev;
    const long long ncol = a->ncol, n2 = (long long)ntime * ncol;
    const bool ref = a->ref_dtype != 0, local = a->local_p_ref != 0;
    NEED(ctx, !ctx->reduce_fn, "latitude-band sharding needs the multi-pass loop (i_reinterp = 0)");
    int rc;
    void *evap = nullptr, *relhum = nullptr, *hur = a->hur_pgw_out;
    const size_t field = (size_t)ntime * N * ncol * elem_size(ref ? PGW_F64 : dtype);      // a level array the loop produces
    if ((rc = ws_get(ctx, 0, field, &evap))) return rc;
    if ((rc = ws_get(ctx, 2, field, &relhum))) return rc;
    if (!hur && (rc = ws_get(ctx, 7, field, &hur))) return rc;
    LoopState ls;
    if ((rc = loop_state(ctx, n2, &ls))) return rc;
    Levels lv = levels_of(ctx);
    const int full_column = ctx->opt[PGW_OPT_FULL_COLUMN];
    const double zx_hi = a->per_var_time ? a->zg_x_hi : a->x_hi, zx_new = a->per_var_time ? a->zg_x_new : a->x_new;
    if (local) NEED(ctx, a->zg3_b != nullptr, "local_p_ref needs the full zg records (zg3_b / zg3_a)");
    ZgAxis zax = {0, nullptr};
    if (local && (rc = zg_axis(ctx, a, &zax))) return rc;
    const PlevTable ptf = file_order_table(zax.n, zax.plev);
    if ((rc = status_reset(ctx))) return rc;
    // ---- ERA state: RELHUM (step_03:87-94)
    {
        Prof pr(ctx, PGW_K_Q_TO_RH);
        if (ref) {
            hipLaunchKernelGGL(k_relhum_ref, dim3(nblocks(n2, BLOCK)), dim3(BLOCK), 0, ctx->stream, lv, ntime, ncol,
                               (const float *)a->QV, (const float *)a->PS, (const float *)a->T, (double *)relhum);
        } else {
            int vec = pick_vec(ctx, dtype, ncol, {a->QV, a->PS, a->T, relhum});
            with_type_vec(dtype, vec, [&](auto t_, auto v_) {
                using T = decltype(t_);
                constexpr int V = decltype(v_)::value;
                hipLaunchKernelGGL((k_humidity_hybrid<T, V, 0>), dim3(nblocks(n2 / V, BLOCK)), dim3(BLOCK), 0, ctx->stream, lv, ntime,
                                   ncol, (const T *)a->QV, (const T *)a->PS, (const T *)a->T, (T *)relhum);
            });
        }
    }
    if (!local) {
        // phi_ref of the ERA state (constant for a fixed p_ref; :280-287 recomputes it) and g * dzg (:292-295); zeroed state
        launch_phi_ref_hybrid(ctx, dtype, ntime, ncol, a->T, a->QV, a->PS, a->FIS, a->p_ref, ls.phi_era, full_column, nullptr, ref);
        launch_dphi_clim(ctx, dtype, ref, n2, a->zg_b, a->zg_a, zx_hi, zx_new, ls);
    } else {
        HIPCHK(ctx, hipMemsetAsync(ls.delta_ps, 0, sizeof(double) * 2 * n2, ctx->stream));    // :182-184
    }
    HIPCHK(ctx, hipGetLastError());
    if ((rc = status_check(ctx))) return rc;

    // one pair of variables (ERA fields + deltas) onto the levels of ps_pgw; thermo: ta + hur with e, else ua + va
    auto reinterp = [&](bool thermo) {
        Prof pr(ctx, PGW_K_VERT_INTERP_DELTA);
        // storage T of the files; TE1, TO: the second ERA field and the outputs (reference-dtype mode: float64 beside float32)
        auto launch = [&](auto t_, auto e1_, auto o_, auto ref_) {
            using T = decltype(t_); using TE1 = decltype(e1_); using TO = decltype(o_);
            ReinterpPair<T, T, TE1, TO> rv;
            rv.d[0] = delta_src<T>(thermo ? a->ta_b : a->ua_b, thermo ? a->ta_a : a->ua_a, a->x_hi, a->x_new);
            rv.d[1] = delta_src<T>(thermo ? a->hur_b : a->va_b, thermo ? a->hur_a : a->va_a, a->x_hi, a->x_new);
            rv.sfc[0] = delta_src<T>(thermo ? a->tas_b : nullptr, thermo ? a->tas_a : nullptr, a->x_hi, a->x_new);
            rv.sfc[1] = delta_src<T>(thermo ? a->hurs_b : nullptr, thermo ? a->hurs_a : nullptr, a->x_hi, a->x_new);
            rv.era0 = (const T *)(thermo ? a->T : a->U); rv.era1 = (const TE1 *)(thermo ? relhum : a->V);
            rv.out[0] = (TO *)(thermo ? a->T_out : a->U_out); rv.out[1] = (TO *)(thermo ? hur : a->V_out);
            rv.evap = thermo ? (TO *)evap : nullptr;
            launch_reinterp_pair<T, T, TE1, TO, decltype(ref_)::value>(ctx, lv, ntime, S, ncol, rv,
                                                                       delta_src<T>(a->pshist_b, a->pshist_a, a->x_hi, a->x_new),
                                                                       (const T *)a->PS, (const T *)a->PS_out, thermo, check_top);
        };
        if (!ref) with_type(dtype, [&](auto t_) { launch(t_, t_, t_, std::false_type()); });
        else if (thermo) launch(float(), double(), double(), std::true_type());      // RELHUM of the ERA state is float64
        else launch(float(), float(), double(), std::true_type());
    };

    LoopControl lc = file_loop_control(a);
    // :186, 189: the reference enters the loop on inf > thresh (no pass at all for a threshold of inf or NaN)
    LoopControl::Verdict verdict = INFINITY > lc.thresh ? LoopControl::CONTINUE : LoopControl::CONVERGED;
    while (verdict == LoopControl::CONTINUE) {
        if ((rc = status_reset(ctx))) return rc;
        if (local) launch_local_p_ref(ctx, dtype, ref, ptf, n2, ncol, a->PS, a->zg3_b, a->zg3_a, zx_hi, zx_new, lc.n_iter() == 0 ? 1 : 0, ls);
        // ps_pgw of this pass; fixed p_ref: after delta_ps += adj_ps   :192-193
        with_flow(dtype, ref, [&](auto t_, auto, auto ref_) {
            using T = decltype(t_);
            hipLaunchKernelGGL((k_update_ps<T, decltype(ref_)::value>), dim3(nblocks(n2, BLOCK)), dim3(BLOCK), 0, ctx->stream, n2,
                               (const T *)a->PS, ls.delta_ps, ls.adj_ps, (T *)a->PS_out, local ? 0 : 1);
        });
        if (local)
            launch_phi_ref_hybrid(ctx, dtype, ntime, ncol, a->T, a->QV, a->PS, a->FIS, 0.0, ls.phi_era, full_column, ls.pref_f, ref);   // :280-287
        reinterp(true);                                                     // :202-216 + e of functions.py:123
        // :262-308 on the re-interpolated fields (delta_ps already carries this pass's increment)
        launch_step(ctx, dtype, ntime, ncol, a->T_out, evap, a->PS, a->FIS, ls.phi_era, ls.dphi, ls.delta_ps, ls.adj_ps, a->p_ref,
                    local ? ls.pref_f : nullptr, a->adj_factor, full_column, 0, nullptr, nullptr, ref);
        HIPCHK(ctx, hipGetLastError());
        if ((rc = status_check(ctx))) return rc;
        if ((rc = top_pressure_check(ctx, !check_top))) return rc;
        verdict = lc.record(max_err_of(ctx));                               // :308-319
    }
    if ((rc = loop_end(ctx, lc, verdict, &a->n_iter))) return rc;
    a->passes_launched = lc.n_iter();
    a->levels_touched = 0;
    if ((rc = status_reset(ctx))) return rc;
    reinterp(false);                                                        // ua, va on the final levels   :330-343
    // hus of the last pass (:262-266, 370) from its e; PS_out already holds ps_pgw of the last pass
    launch_finalize(ctx, dtype, ref, ntime, ncol, a->PS, ls.delta_ps, evap, a->PS_out, a->QV_out, 0);
    HIPCHK(ctx, hipGetLastError());
    if ((rc = status_check(ctx))) return rc;
    return top_pressure_check(ctx, !check_top);
}

// ------------------------------------------------------------------ whole file
static int step03_file(pgw_ctx *ctx, pgw_file_args *a);

extern "C" int pgw_step03_file(pgw_ctx *ctx, pgw_file_args *a) {
    if (!ctx) return PGW_ERR_ARG;
    ctx->band_reduces = 0; ctx->band_next_np = 0; ctx->band_agreed = false;
    const int rc = step03_file(ctx, a);
    // latitude-band mode: whatever made this band stop on its own - an argument check, a failed allocation, a data error
    // before the loop, a HIP error between two loop launches - reaches the other bands through their next reduce
    return (rc != PGW_OK && ctx->reduce_fn) ? band_fail(ctx, rc, a ? a->max_n_iter : 1) : rc;
}

// ------------------------------------------------------------------ record bracketing on the host (functions.py:224-283)
// Civil dates of the proleptic Gregorian calendar from days since 1970-01-01 and back (the usual era-of-400-years pair);
// floor semantics before 1970 like numpy's datetime64 casts.
static long long floor_div(long long a, long long b) { return a / b - ((a % b != 0) && ((a < 0) != (b < 0))); }

static long long days_from_civil(long long y, int m, int d) {
    y -= m <= 2;
    const long long era = floor_div(y, 400);
    const long long yoe = y - era * 400;
    const long long doy = (153 * (m + (m > 2 ? -3 : 9)) + 2) / 5 + d - 1;
    const long long doe = yoe * 365 + yoe / 4 - yoe / 100 + doy;
    return era * 146097 + doe - 719468;
}

static void civil_from_days(long long z, long long *y, int *m, int *d) {
    z += 719468;
    const long long era = floor_div(z, 146097);
    const long long doe = z - era * 146097;
    const long long yoe = (doe - doe / 1460 + doe / 36524 - doe / 146096) / 365;
    const long long doy = doe - (365 * yoe + yoe / 4 - yoe / 100);
    const long long mp = (5 * doy + 2) / 153;
    *d = (int)(doy - (153 * mp + 2) / 5 + 1);
    *m = (int)(mp < 10 ? mp + 3 : mp - 9);
    *y = yoe + era * 400 + (*m <= 2);
}

// `dt64_to_dt(t).replace(year=year)` as the array form states it: first second of (year, month of t) + offset of t in its month
static long long reyear(long long t, long long year) {
    long long y; int m, d;
    civil_from_days(floor_div(t, 86400), &y, &m, &d);
    return days_from_civil(year, m, 1) * 86400 + (t - days_from_civil(y, m, 1) * 86400);
}

extern "C" int pgw_delta_bracket(const long long *times_s, int n, long long target_s, int *ind_before, int *ind_after,
                                 double *x_hi, double *x_new, int *dropped) {
    if (!times_s || !ind_before || !ind_after || !x_hi || !x_new || !dropped || n < 1) return PGW_ERR_ARG;
    int leap = -1;                                                  // :224-230: the LAST Feb 29 found is dropped
    for (int i = 0; i < n; ++i) {
        long long y; int m, d;
        civil_from_days(floor_div(times_s[i], 86400), &y, &m, &d);
        if (m == 2 && d == 29) leap = i;
    }
    const int nk = n - (leap >= 0);
    if (nk < 1) return PGW_ERR_ARG;
    long long year; int tm, td;
    civil_from_days(floor_div(target_s, 86400), &year, &tm, &td);
    int ib = -1, ia = -1, k = 0;
    long long tb = 0, ta = 0, first = 0, last = 0;
    for (int i = 0; i < n; ++i) {
        if (i == leap) continue;
        const long long ty = reyear(times_s[i], year);              // :235-238
        if (k == 0) first = ty;
        last = ty;
        if (ty <= target_s) { ib = k; tb = ty; }                    // :242-243: the last one at or before
        if (ty >= target_s && ia < 0) { ia = k; ta = ty; }          // :262-263: the first one at or after
        ++k;
    }
    if (ib < 0) { ib = nk - 1; tb = reyear(last, year - 1); }       // :253-258
    if (ia < 0) { ia = 0; ta = reyear(first, year + 1); }           // :273-278
    *ind_before = ib; *ind_after = ia; *dropped = leap;
    if (ib == ia) { *x_hi = 0.0; *x_new = 0.0; }                    // :282-283
    else {
        *x_hi = (double)((ta - tb) * 1000000000LL);
        *x_new = (double)((target_s - tb) * 1000000000LL);
    }
    return PGW_OK;
}

// ------------------------------------------------------------------ whole file from a plan
extern "C" int pgw_step03_file_at(pgw_ctx *ctx, const pgw_file_plan *plan, long long target_s, pgw_file_args *filled) {
    if (!ctx) return PGW_ERR_ARG;
    NEED(ctx, plan != nullptr && filled != nullptr, "null plan or args");
    NEED(ctx, plan->n_axes >= 1 && plan->n_axes <= PGW_PLAN_MAX_AXES, "bad number of time axes");
    NEED(ctx, plan->args.per_var_time != 0, "the plan's template must have per_var_time = 1");
    struct { int ib, ia; double x_hi, x_new; } br[PGW_PLAN_MAX_AXES];
    for (int i = 0; i < plan->n_axes; ++i) {
        int ib, ia, drop;
        NEED(ctx, pgw_delta_bracket(plan->axis_times[i], plan->axis_len[i], target_s, &ib, &ia, &br[i].x_hi, &br[i].x_new,
                                    &drop) == PGW_OK, "time axis without a usable stamp");
        br[i].ib = ib + (drop >= 0 && ib >= drop);                  // kept index -> record
        br[i].ia = ia + (drop >= 0 && ia >= drop);
    }
    *filled = plan->args;
    pgw_file_args *a = filled;
    const void **slot_b[PGW_PV_COUNT] = {&a->ta_b, &a->hur_b, &a->ua_b, &a->va_b, &a->tas_b, &a->hurs_b, &a->pshist_b,
                                         a->local_p_ref ? &a->zg3_b : &a->zg_b, &a->siconc_b, &a->ts_b, &a->tos_b};
    const void **slot_a[PGW_PV_COUNT] = {&a->ta_a, &a->hur_a, &a->ua_a, &a->va_a, &a->tas_a, &a->hurs_a, &a->pshist_a,
                                         a->local_p_ref ? &a->zg3_a : &a->zg_a, &a->siconc_a, &a->ts_a, &a->tos_a};
    double *own_hi[PGW_PV_COUNT] = {}, *own_new[PGW_PV_COUNT] = {};  // abscissae of the variables bracketed on their own
    own_hi[PGW_PV_ZG] = &a->zg_x_hi;         own_new[PGW_PV_ZG] = &a->zg_x_new;
    own_hi[PGW_PV_SICONC] = &a->siconc_x_hi; own_new[PGW_PV_SICONC] = &a->siconc_x_new;
    own_hi[PGW_PV_TS] = &a->ts_x_hi;         own_new[PGW_PV_TS] = &a->ts_x_new;
    own_hi[PGW_PV_TOS] = &a->tos_x_hi;       own_new[PGW_PV_TOS] = &a->tos_x_new;
    const pgw_plan_var *ta = &plan->var[PGW_PV_TA];
    NEED(ctx, ta->base != nullptr, "the plan has no ta records");
    for (int v = 0; v < PGW_PV_COUNT; ++v) {
        const pgw_plan_var *pv = &plan->var[v];
        if (!pv->base) continue;
        NEED(ctx, pv->axis >= 0 && pv->axis < plan->n_axes, "variable on an axis the plan does not have");
        NEED(ctx, v > PGW_PV_PS_HIST || pv->axis == ta->axis, "the quad group must share ta's time axis");
        const char *base = (const char *)pv->base + (a->local_p_ref ? 0 : pv->ref_offset);
        *slot_b[v] = base + (long long)br[pv->axis].ib * pv->rec_bytes;
        *slot_a[v] = base + (long long)br[pv->axis].ia * pv->rec_bytes;
        if (own_hi[v]) { *own_hi[v] = br[pv->axis].x_hi; *own_new[v] = br[pv->axis].x_new; }
    }
    a->x_hi = br[ta->axis].x_hi;
    a->x_new = br[ta->axis].x_new;
    return pgw_step03_file(ctx, a);
}

static int step03_file(pgw_ctx *ctx, pgw_file_args *a) {
    NEED(ctx, a != nullptr, "null args");
    const int dtype = a->dtype, ntime = a->ntime;
    const long long ncol = a->ncol;
    CHECK_COMMON(ctx, dtype, ntime, ncol);
    NEED(ctx, ctx->nlev > 0 && a->nlev == ctx->nlev, "nlev must match pgw_set_levels");
    NEED(ctx, a->nplev >= 2 && a->nplev <= MAX_PLEV_WIDE, PLEV_RANGE_2);
    NEED(ctx, a->PS && a->FIS && a->T && a->QV && a->U && a->V, "ERA5 field pointer is NULL");
    NEED(ctx, a->plev && a->ta_b && a->hur_b && a->ua_b && a->va_b && (a->zg_b || a->local_p_ref) && a->tas_b && a->hurs_b &&
         a->pshist_b, "delta record pointer is NULL");
    NEED(ctx, a->PS_out && a->T_out && a->QV_out && a->U_out && a->V_out, "output pointer is NULL");
    NEED(ctx, a->max_n_iter >= 1 && a->max_n_iter <= 1000, "bad max_n_iter");
    NEED(ctx, !ctx->reduce_fn || (ctx->opt[PGW_OPT_MULTIPASS] && !ctx->opt[PGW_OPT_FULL_COLUMN]),
         "a reduce hook (latitude-band sharding) needs the multi-pass loop: PGW_OPT_MULTIPASS = 1, PGW_OPT_FULL_COLUMN = 0");
    const bool ref = a->ref_dtype != 0;
    NEED(ctx, !ref || dtype == PGW_F32, "ref_dtype = 1 is the float32-file mode: dtype must be PGW_F32");
    NEED(ctx, !ref || ctx->opt[PGW_OPT_QUAD], "ref_dtype = 1 needs the quad kernel (PGW_OPT_QUAD = 1)");
    const int N = a->nlev;
    int rc;
    ZgAxis zax = {0, nullptr};                            // local_p_ref: checked before anything is launched
    if (a->local_p_ref && (rc = zg_axis(ctx, a, &zax))) return rc;
    int qv_done = 0;          // leading levels whose final QV the quad kernel has already written
    // PGW_OPT_FUSED_FIRST: the quad kernel runs the first two scans of the multi-pass loop with a fixed p_ref.  float64
    // storage only: the float32 instantiations of the quad kernel lose more than the loop kernel gains
    const bool fused_first = dtype == PGW_F64 && ctx->opt[PGW_OPT_FUSED_FIRST] && ctx->opt[PGW_OPT_QUAD] && ctx->opt[PGW_OPT_MULTIPASS] &&
                           !ctx->opt[PGW_OPT_FULL_COLUMN] && !a->local_p_ref && !a->i_reinterp;
    if ((rc = plev_table(ctx, a->nplev, a->plev))) return rc;
    void *evap = nullptr;      // PGW level arrays (evap, 4-D outputs): float64 in reference-dtype mode
    if ((rc = ws_get(ctx, 0, (size_t)ntime * N * ncol * elem_size(ref ? PGW_F64 : dtype), &evap))) return rc;
    Levels lv = levels_of(ctx);
    const int check_top = a->ignore_top ? 0 : 1;
    // each delta file has its own time axis in the reference (load_delta per variable): own bracket, own abscissae
    const double zx_hi = a->per_var_time ? a->zg_x_hi : a->x_hi, zx_new = a->per_var_time ? a->zg_x_new : a->x_new;

    // ---- surface riders (step_03:103-146): independent of everything else in the file.  On the production path
    // (PGW_OPT_FINISH_IN_PASS) the multi-pass loop enqueues them behind its first launch's status read-back; otherwise here
    std::function<int()> riders;
    if (a->FR_SEA_ICE && a->siconc_b && a->FR_SEA_ICE_out) {
        NEED(ctx, a->ts_b && a->tos_b && a->FR_LAND && a->T_SKIN && a->T_SKIN_out, "surface rider pointer is NULL");
        SoilTable st;
        if ((rc = soil_table(ctx, __func__, a->nsoil, a->soil_depth, &st))) return rc;
        NEED(ctx, a->nsoil == 0 || (a->T_SO && a->T_SO_out && a->ts_clim && a->soil_depth), "soil pointers missing");
        riders = [ctx, a, st, dtype, ref, ntime, ncol]() {
            long long n = (long long)ntime * ncol;
            Prof pr(ctx, PGW_K_SURFACE);
            with_flow(dtype, ref, [&](auto t_, auto, auto ref_) {
                using T = decltype(t_);
                const bool own = a->per_var_time != 0;
                const DeltaSrc<T> dsic = delta_src<T>(a->siconc_b, a->siconc_a, own ? a->siconc_x_hi : a->x_hi, own ? a->siconc_x_new : a->x_new);
                const DeltaSrc<T> dts = delta_src<T>(a->ts_b, a->ts_a, own ? a->ts_x_hi : a->x_hi, own ? a->ts_x_new : a->x_new);
                const DeltaSrc<T> dtos = delta_src<T>(a->tos_b, a->tos_a, own ? a->tos_x_hi : a->x_hi, own ? a->tos_x_new : a->x_new);
                const RiderSrc<T> r{(const T *)a->FR_SEA_ICE, dsic, dtos, dts, (const T *)a->FR_LAND};
                hipLaunchKernelGGL((k_surface_update_lerp<T, decltype(ref_)::value>), dim3(nblocks(n, BLOCK)), dim3(BLOCK), 0, ctx->stream,
                                   ntime, ncol, st, r, (const T *)a->ts_clim, (const T *)a->T_SKIN, (const T *)a->T_SO,
                                   (T *)a->FR_SEA_ICE_out, (T *)nullptr /* comb_out */, (T *)a->T_SKIN_out, (T *)a->T_SO_out);
            });
            HIPCHK(ctx, hipGetLastError());
            return (int)PGW_OK;
        };
        const bool behind_loop = ctx->opt[PGW_OPT_FINISH_IN_PASS] && ctx->opt[PGW_OPT_QUAD] && ctx->opt[PGW_OPT_MULTIPASS] &&
                                 !ctx->opt[PGW_OPT_FULL_COLUMN] && !a->local_p_ref && !a->i_reinterp;
        if (!behind_loop) {
            if ((rc = riders())) return rc;
            riders = nullptr;
        }
    }

    if (a->i_reinterp) {                                  // settings.i_reinterp = 1: the loop re-interpolates in every pass
        a->levels_touched = 0; a->passes_launched = 0;
        ctx->last_qv_from_pass = false; ctx->last_qv_skipped = 0;
        return run_reinterp_file(ctx, a, check_top);
    }

    // ---- ta + hur -> T_pgw, e_pgw   and   ua + va -> U_pgw, V_pgw
    // One column per thread: these kernels are bound by fp64 VALU work and register footprint, not by load width.
    {
        const int S = a->nplev;
        // one host synchronisation per file: without the model-top check nothing has to be read back
        // between the kernels (errors stay in the status block until the loop's first check)
        const bool defer = !check_top && !a->local_p_ref;
        if ((rc = status_reset(ctx))) return rc;
        if (ctx->opt[PGW_OPT_QUAD]) {
            // ---- all four variables in one kernel (production)
            const size_t qlds = (size_t)(5 * N + 2) * sizeof(double);
            qv_done = ctx->opt[PGW_OPT_FULL_COLUMN] ? 0 : ctx->n_pure;     // full-column passes read e at every level
            LoopState ls;
            memset(&ls, 0, sizeof(ls));
            void *dps_hist = nullptr;
            if (fused_first) {
                // the delta kernel writes into the loop's state: the workspace and the armed status block come first
                if ((rc = loop_state(ctx, (long long)ntime * ncol, &ls))) return rc;
                if ((rc = ws_get(ctx, 6, (size_t)ntime * ncol * MULTI_MAX_PASS * sizeof(double), &dps_hist))) return rc;
                // blocks 1 (errors of the kernel's ERA-state scan) and 2 (pass 1) of the device status
                HIPCHK(ctx, hipMemcpyAsync(ctx->d_status + 1, blank_blocks(ctx, 2), 2 * sizeof(DevStatus), hipMemcpyHostToDevice, ctx->stream));
            }
            {
                Prof pr(ctx, PGW_K_QUAD_DELTA);
                hipError_t copied = hipSuccess;
                with_flow(dtype, ref, [&](auto t_, auto l_, auto ref_) {
                    using T = decltype(t_); using TL = decltype(l_);
                    const FusedFirst<T> ff{a->adj_factor, (const T *)a->FIS, delta_src<T>(a->zg_b, a->zg_a, zx_hi, zx_new),
                                           ls.phi_era, ls.dphi, ls.delta_ps, ls.adj_ps, (double *)dps_hist, ls.era_flags,
                                           ctx->d_status + 1, ctx->d_status + 2};
                    // the kernel reads the block from device memory (the host copy is free again after this file's read-back)
                    static_assert(sizeof(FusedFirst<T>) <= FUSED_BLOCKS * sizeof(DevStatus), "FusedFirst block");
                    FusedFirst<T> *h_ff = (FusedFirst<T> *)(ctx->h_status + 2 + 2 * MULTI_MAX_PASS);
                    const FusedFirst<T> *d_ff = (const FusedFirst<T> *)(ctx->d_status + 2 + MULTI_MAX_PASS);
                    if (fused_first) {
                        *h_ff = ff;
                        copied = hipMemcpyAsync((void *)d_ff, h_ff, sizeof(ff), hipMemcpyHostToDevice, ctx->stream);
                        if (copied != hipSuccess) return;
                    }
                    const PairSrc<T> dth = pair_src<T>(a->ta_b, a->ta_a, a->hur_b, a->hur_a, a->x_hi, a->x_new);
                    const PairSrc<T> ds = pair_src<T>(a->tas_b, a->tas_a, a->hurs_b, a->hurs_a, a->x_hi, a->x_new);
                    const DeltaSrc<T> ph = delta_src<T>(a->pshist_b, a->pshist_a, a->x_hi, a->x_new);
                    const PairSrc<T> dwd = pair_src<T>(a->ua_b, a->ua_a, a->va_b, a->va_a, a->x_hi, a->x_new);
                    // O: arrays below 4 GiB (a 0.25 deg L137 field is 1.1 GB): 32-bit byte offsets from uniform bases
                    // LERP: the instant lies between two records (false: it is a record); FUSE: fused_first
                    auto launch = [&](auto o_, auto lerp_, auto fuse_) { with_plev(ctx, [&](const auto &pt) {
                        hipLaunchKernelGGL((k_delta_quad<T, TL, QUAD_U, QUAD_TPB, decltype(o_), decltype(lerp_)::value != 0, decltype(ref_)::value, decltype(fuse_)::value, false, std::decay_t<decltype(pt)>>),
                                           dim3(nblocks((long long)ntime * ncol, QUAD_TPB)), dim3(QUAD_TPB), qlds, ctx->stream, pt,
                                           lv, ntime, ncol, (const T *)a->T, (const T *)a->QV, (const T *)a->U, (const T *)a->V,
                                           (const T *)a->PS, dth, ds, ph, dwd, check_top, (TL *)a->T_out, (TL *)evap,
                                           (TL *)a->hur_pgw_out, (TL *)a->U_out, (TL *)a->V_out, (TL *)a->QV_out, qv_done, ctx->n_pure,
                                           ctx->d_status, a->p_ref, d_ff);
                    }); };
                    const bool o32 = !ctx->opt[PGW_OPT_FORCE_OFF64] &&
                                     (unsigned long long)ntime * (N > S ? N : S) * ncol * sizeof(TL) < (1ull << 32);
                    with_offsets(o32, [&](auto o_) { with_int<2>(a->x_hi != 0.0, [&](auto lerp_) {
                        if constexpr (sizeof(T) == 8) { if (fused_first) return launch(o_, lerp_, std::true_type()); }
                        launch(o_, lerp_, std::false_type());
                    }); });
                });
                if (copied != hipSuccess) return fail(ctx, PGW_ERR_HIP, "hipMemcpyAsync (FusedFirst block)");
            }
            HIPCHK(ctx, hipGetLastError());
        } else {
            // ---- PGW_OPT_QUAD = 0: the two pair kernels the quad kernel replaced (kept as an independently written
            // cross-check of the same arithmetic: tests/test_hip_parity.py::test_kernel_variants_are_bit_identical)
            const size_t lds = (size_t)2 * N * sizeof(double);            // akm | bkm
            const unsigned int grid = nblocks((long long)ntime * ncol, 128);
            {
                Prof pr(ctx, PGW_K_THERMO_DELTA);
                with_type(dtype, [&](auto t_) { with_plev(ctx, [&](const auto &pt) {
                    using T = decltype(t_);
                    hipLaunchKernelGGL((k_delta_pair<T, 1, true, 2, 128, std::decay_t<decltype(pt)>>), dim3(grid), dim3(128), lds, ctx->stream, pt, lv, ntime,
                                       ncol, (const T *)a->T, (const T *)a->QV, (const T *)a->PS,
                                       pair_src<T>(a->ta_b, a->ta_a, a->hur_b, a->hur_a, a->x_hi, a->x_new),
                                       pair_src<T>(a->tas_b, a->tas_a, a->hurs_b, a->hurs_a, a->x_hi, a->x_new),
                                       delta_src<T>(a->pshist_b, a->pshist_a, a->x_hi, a->x_new), check_top, (T *)a->T_out, (T *)evap,
                                       (T *)a->hur_pgw_out, ctx->d_status);
                }); });
            }
            {
                Prof pr(ctx, PGW_K_WIND_DELTA);
                with_type(dtype, [&](auto t_) { with_plev(ctx, [&](const auto &pt) {
                    using T = decltype(t_);
                    hipLaunchKernelGGL((k_delta_pair<T, 1, false, PAIR_U, 128, std::decay_t<decltype(pt)>>), dim3(grid), dim3(128), lds, ctx->stream, pt, lv,
                                       ntime, ncol, (const T *)a->U, (const T *)a->V, (const T *)a->PS,
                                       pair_src<T>(a->ua_b, a->ua_a, a->va_b, a->va_a, a->x_hi, a->x_new),
                                       pair_src<T>(nullptr, nullptr, nullptr, nullptr, 0.0, 0.0), delta_src<T>(nullptr, nullptr, 0.0, 0.0),
                                       check_top, (T *)a->U_out, (T *)a->V_out, (T *)nullptr, ctx->d_status);
                }); });
            }
            HIPCHK(ctx, hipGetLastError());
        }
        if (!defer) {
            if ((rc = status_check(ctx))) return rc;            // (latitude-band mode: pgw_step03_file meets the other bands)
            if ((rc = top_pressure_check(ctx, a->ignore_top))) return rc;
        }
    }

    // ---- fixed-point loop + final PS, QV
    PsLoopArgs la;
    la.n_iter = &a->n_iter; la.ctl = file_loop_control(a);
    if (a->local_p_ref) NEED(ctx, a->zg3_b != nullptr, "local_p_ref needs the full zg records (zg3_b / zg3_a)");
    la.dtype = dtype; la.ntime = ntime; la.ncol = ncol;
    la.PS = a->PS; la.FIS = a->FIS; la.T = a->T; la.QV = a->QV;
    la.ta_pgw = a->T_out; la.evap = evap;
    la.dzg_b = a->local_p_ref ? a->zg3_b : a->zg_b; la.dzg_a = a->local_p_ref ? a->zg3_a : a->zg_a;
    la.x_hi = zx_hi; la.x_new = zx_new;
    la.p_ref = a->p_ref; la.adj_factor = a->adj_factor;
    la.ps_pgw = a->PS_out; la.hus_pgw = a->QV_out;
    if (a->local_p_ref) { la.local_nplev = zax.n; la.plev_file = zax.plev; }
    la.status_armed = !check_top && !a->local_p_ref;
    la.qv_done_levels = qv_done; la.ref = ref; la.fused_first = fused_first;
    la.qv_from_pass = ctx->opt[PGW_OPT_QUAD] != 0;
    la.riders = riders;
    rc = run_ps_loop(ctx, la);
    a->levels_touched = ctx->last_levels_touched;
    a->passes_launched = ctx->last_passes_launched;
    return rc;
}

extern "C" unsigned long long pgw_last_levels_touched(pgw_ctx *ctx) { return ctx->last_levels_touched; }

extern "C" int pgw_last_qv_from_pass(pgw_ctx *ctx, unsigned long long *skipped) {
    if (skipped) *skipped = ctx->last_qv_from_pass ? ctx->last_qv_skipped : 0;
    return ctx->last_qv_from_pass ? 1 : 0;
}

extern "C" int pgw_test_exp(pgw_ctx *ctx, long long n, const double *in, double *out, double *ref) {
    NEED(ctx, n >= 1 && in && out && ref, "bad argument");
    hipLaunchKernelGGL(k_test_exp, dim3(nblocks(n, 256)), dim3(256), 0, ctx->stream, n, in, out, ref);
    HIPCHK(ctx, hipGetLastError());
    return PGW_OK;
}

extern "C" int pgw_test_rh_f32(pgw_ctx *ctx, long long n, const float *hus, const double *pa, const float *ta,
                               double *out, double *lit, float *es, float *es_lit) {
    NEED(ctx, n >= 1 && hus && pa && ta && out && lit && es && es_lit, "bad argument");
    hipLaunchKernelGGL(k_test_rh_f32, dim3(nblocks(n, 256)), dim3(256), 0, ctx->stream, n, hus, pa, ta, out, lit, es, es_lit);
    HIPCHK(ctx, hipGetLastError());
    return PGW_OK;
}

extern "C" int pgw_test_shared_div(pgw_ctx *ctx, long long n, const double *num, const double *den, double *out) {
    NEED(ctx, n >= 1 && num && den && out, "bad argument");
    hipLaunchKernelGGL(k_test_shared_div, dim3(nblocks(n, 256)), dim3(256), 0, ctx->stream, n, num, den, out);
    HIPCHK(ctx, hipGetLastError());
    return PGW_OK;
}

extern "C" int pgw_harmonic_smooth(pgw_ctx *ctx, int dtype, int ntime, long long inner, const double *cos_tab,
                                   const double *sin_tab, const void *in, void *out) {
    NEED(ctx, dtype == PGW_F32 || dtype == PGW_F64, "dtype must be PGW_F32 or PGW_F64");
    NEED(ctx, inner >= 1 && in && out && cos_tab && sin_tab, "bad argument");
    // functions.py:724-737: the first three harmonics need 3 < floor(ntime / 2)
    if (!(3 < ntime / 2))
        return fail(ctx, PGW_ERR_ARG, "Whooops that should not be the case for a yearly timeseries! i (reconstruction grade) "
                                      "is larger than the number of timeseries elements / 2.");
    const size_t lds = sizeof(double) * 6 * (size_t)ntime;
    NEED(ctx, lds <= 64 * 1024, "time series longer than 1365 steps are not supported");
    void *tab = nullptr;
    int rc = ws_get(ctx, 5, lds, &tab);
    if (rc) return rc;
    HIPCHK(ctx, hipMemcpyAsync(tab, cos_tab, lds / 2, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync((char *)tab + lds / 2, sin_tab, lds / 2, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));                  // the host tables may be freed after the call
    {
        Prof pr(ctx, PGW_K_HARMONIC);
        with_type(dtype, [&](auto t_) {
            using T = decltype(t_);
            hipLaunchKernelGGL((k_harmonic_smooth<T, 8>), dim3(nblocks(inner, BLOCK)), dim3(BLOCK), lds, ctx->stream, ntime, inner,
                               (const double *)tab, (const T *)in, (T *)out);
        });
    }
    HIPCHK(ctx, hipGetLastError());
    return PGW_OK;
}

// What pgw_gauss_interp and pgw_gauss_interp_points ask of their arguments alike (`caller` names the entry in the status text),
// and the constants their kernels take: radius^2, vtkGaussianKernel's F2 = (Sharpness / Radius)^2, cells per metre
struct GaussParams { double r2, f2, inv_h; };
static int gauss_args(pgw_ctx *ctx, const char *caller, long long ntarg, const double *tx, const double *ty, int ncx, int ncy,
                      double cell, const int *cell_start, long long nsrc, const double *sx, const double *sy, const double *sval,
                      int nfield, double radius, double sharpness, const double *out, GaussParams *g) {
    NEED_AS(ctx, caller, ntarg >= 1 && nsrc >= 0 && tx && ty && cell_start && out, "bad argument");
    NEED_AS(ctx, caller, nsrc == 0 || (sx && sy && sval), "null source pointer");
    NEED_AS(ctx, caller, ncx >= 1 && ncy >= 1 && cell > 0.0 && radius > 0.0, "bad cell grid");
    NEED_AS(ctx, caller, cell >= radius, "cells must be at least one kernel radius wide (3 x 3 block search)");
    NEED_AS(ctx, caller, nfield >= 1 && nfield <= GAUSS_MAX_FIELDS, "nfield must be in [1, 16]");
    *g = {radius * radius, (sharpness * sharpness) / (radius * radius), 1.0 / cell};
    return PGW_OK;
}

extern "C" int pgw_gauss_interp(pgw_ctx *ctx, long long ntarg, const double *tx, const double *ty, int ncx, int ncy,
                                double x0, double y0, double cell, const int *cell_start, long long nsrc, const double *sx,
                                const double *sy, const double *sval, int nfield, double radius, double sharpness, double *out) {
    GaussParams g;
    if (int rc = gauss_args(ctx, __func__, ntarg, tx, ty, ncx, ncy, cell, cell_start, nsrc, sx, sy, sval, nfield, radius, sharpness, out, &g)) return rc;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    {
        Prof pr(ctx, PGW_K_GAUSS_INTERP);
        hipLaunchKernelGGL((k_gauss_interp<GAUSS_MAX_FIELDS>), dim3(nblocks(ntarg, BLOCK)), dim3(BLOCK), 0, ctx->stream, ntarg, tx, ty,
                           ncx, ncy, x0, y0, g.inv_h, cell_start, sx, sy, sval, nfield, g.r2, g.f2, out);
    }
    HIPCHK(ctx, hipGetLastError());
    return PGW_OK;
}

extern "C" int pgw_planar_metres(pgw_ctx *ctx, long long n, const double *lat, const double *lon, double *lat_m, double *lon_m,
                                 double *lon_off) {
    NEED(ctx, n >= 0 && (n == 0 || (lat && lon && lat_m && lon_m && lon_off)), "bad argument");
    if (n == 0) return PGW_OK;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    hipLaunchKernelGGL(k_planar_metres, dim3(nblocks(n, BLOCK)), dim3(BLOCK), 0, ctx->stream, n, lat, lon, lat_m, lon_m, lon_off);
    HIPCHK(ctx, hipGetLastError());
    return PGW_OK;
}

extern "C" int pgw_ocean_targets(pgw_ctx *ctx, long long n, const double *lat, const double *lon, const double *land, double *tx,
                                 double *ty) {
    NEED(ctx, n >= 0 && (n == 0 || (lat && lon && tx && ty)), "bad argument");
    if (n == 0) return PGW_OK;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    hipLaunchKernelGGL(k_ocean_targets, dim3(nblocks(n, BLOCK)), dim3(BLOCK), 0, ctx->stream, n, lat, lon, land, tx, ty);
    HIPCHK(ctx, hipGetLastError());
    return PGW_OK;
}

extern "C" int pgw_gauss_interp_points(pgw_ctx *ctx, long long ntarg, const double *tx, const double *ty, int ncx, int ncy,
                                       double x0, double y0, double cell, const int *cell_start, long long nsrc, const double *sx,
                                       const double *sy, const double *sval, int nfield, double radius, double sharpness,
                                       double *out) {
    GaussParams g;
    if (int rc = gauss_args(ctx, __func__, ntarg, tx, ty, ncx, ncy, cell, cell_start, nsrc, sx, sy, sval, nfield, radius, sharpness, out, &g)) return rc;
    NEED(ctx, ntarg < (1ll << 31), "ntarg must be below 2^31 (the order of the targets is kept in 32-bit indices)");
    // keys: the cells and a ring around them, GAUSS_SUB x GAUSS_SUB parts of each, and one for the inactive targets
    const long long nkey = ((long long)ncx + 2) * ((long long)ncy + 2) * (GAUSS_SUB * GAUSS_SUB) + 1;
    NEED(ctx, nkey < (1ll << 31), "16 * (ncx + 2) * (ncy + 2) must be below 2^31");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    // workspace: n_active (and padding) | key [ntarg] | order [ntarg] | count -> start [nkey]
    void *wsp = nullptr;
    if (int rc = ws_get(ctx, 8, sizeof(int) * (4 + 2 * (size_t)ntarg + (size_t)nkey), &wsp)) return rc;
    int *n_active = (int *)wsp, *key = n_active + 4, *order = key + ntarg, *count = order + ntarg;
    const unsigned int nb = nblocks(ntarg, BLOCK);
    HIPCHK(ctx, hipMemsetAsync(count, 0, sizeof(int) * (size_t)nkey, ctx->stream));
    hipLaunchKernelGGL(k_gauss_keys, dim3(nb), dim3(BLOCK), 0, ctx->stream, (int)ntarg, tx, ty, ncx, ncy, x0, y0, g.inv_h, key, count);
    hipLaunchKernelGGL(k_gauss_scan, dim3(1), dim3(SCAN_BLOCK), 0, ctx->stream, (int)nkey, count, n_active);
    hipLaunchKernelGGL(k_gauss_scatter, dim3(nb), dim3(BLOCK), 0, ctx->stream, (int)ntarg, key, count, order);
    HIPCHK(ctx, hipGetLastError());
    {
        Prof pr(ctx, PGW_K_GAUSS_INTERP);
        hipLaunchKernelGGL((k_gauss_points<GAUSS_MAX_FIELDS>), dim3(nb), dim3(BLOCK), 0, ctx->stream, (int)ntarg, order, n_active, tx, ty,
                           ncx, ncy, x0, y0, g.inv_h, cell_start, sx, sy, sval, nfield, g.r2, g.f2, out);
    }
    HIPCHK(ctx, hipGetLastError());
    return PGW_OK;
}

extern "C" int pgw_placement_probe(pgw_ctx *ctx, int n_src, const void *const *src, int n_dst, void *const *dst, long long rows,
                                   long long ncol, int reps, double *gbps) {
    NEED(ctx, n_src >= 0 && n_src <= 4 && n_dst >= 0 && n_dst <= 4 && n_src + n_dst > 0, "1 to 4 + 4 streams");
    NEED(ctx, rows > 0 && ncol > 0 && reps > 0 && gbps, "bad argument");
    ProbeStreams s;
    s.ns = n_src; s.nd = n_dst;
    for (int i = 0; i < 4; ++i) {
        s.src[i] = i < n_src ? (const double *)src[i] : nullptr;
        s.dst[i] = i < n_dst ? (double *)dst[i] : nullptr;
        NEED(ctx, (i >= n_src || (s.src[i] && ((uintptr_t)s.src[i] % 8) == 0)) && (i >= n_dst || (s.dst[i] && ((uintptr_t)s.dst[i] % 8) == 0)),
             "stream pointers must be non-null and 8-byte aligned");
    }
    HIPCHK(ctx, hipSetDevice(ctx->device));
    hipEvent_t e0 = nullptr, e1 = nullptr;             // its own pair: pgw_timer_start / _stop of the caller stay untouched
    HIPCHK(ctx, hipEventCreate(&e0));
    if (hipEventCreate(&e1) != hipSuccess) { hipEventDestroy(e0); return fail(ctx, PGW_ERR_HIP, "hipEventCreate failed"); }
    const unsigned int nb = nblocks(ncol, 128);
    hipLaunchKernelGGL(k_placement_probe, dim3(nb), dim3(128), 0, ctx->stream, rows, ncol, s);       // warm-up
    hipError_t e = hipEventRecord(e0, ctx->stream);
    for (int i = 0; i < reps; ++i) hipLaunchKernelGGL(k_placement_probe, dim3(nb), dim3(128), 0, ctx->stream, rows, ncol, s);
    if (e == hipSuccess) e = hipEventRecord(e1, ctx->stream);
    if (e == hipSuccess) e = hipEventSynchronize(e1);
    if (e == hipSuccess) e = hipGetLastError();
    float ms = 0.f;
    if (e == hipSuccess) e = hipEventElapsedTime(&ms, e0, e1);
    hipEventDestroy(e0); hipEventDestroy(e1);
    if (e != hipSuccess) return fail(ctx, PGW_ERR_HIP, "placement probe failed: %s", hipGetErrorString(e));
    *gbps = ms > 0.f ? (double)rows * (double)ncol * 8.0 * (n_src + n_dst) * reps / ((double)ms * 1e6) : 0.0;
    return PGW_OK;
}

extern "C" int pgw_ws_adopt(pgw_ctx *ctx, int slot, void *dptr, size_t bytes) {
    NEED(ctx, slot >= 0 && slot < 8, "workspace slot out of range");
    NEED(ctx, (dptr != nullptr) == (bytes > 0), "a buffer and its size, or neither (release the slot)");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    if (ctx->ws[slot] && ctx->ws[slot] != dptr) {
        HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
        HIPCHK(ctx, hipFree(ctx->ws[slot]));
    }
    ctx->ws[slot] = dptr; ctx->ws_bytes[slot] = bytes;
    return PGW_OK;
}

extern "C" int pgw_byteswap(pgw_ctx *ctx, int elem_bytes, long long n, const void *src, void *dst) {
    NEED(ctx, elem_bytes == 4 || elem_bytes == 8, "elem_bytes must be 4 or 8");
    NEED(ctx, n >= 0 && (n == 0 || (src && dst)), "bad argument");
    if (n == 0) return PGW_OK;
    NEED(ctx, ((uintptr_t)src % elem_bytes) == 0 && ((uintptr_t)dst % elem_bytes) == 0, "pointers must be element-aligned");
    const bool al16 = ((uintptr_t)src % 16) == 0 && ((uintptr_t)dst % 16) == 0;
    const long long n16 = al16 ? n / (16 / elem_bytes) : 0;
    const long long work = al16 ? (n16 ? n16 : 1) : n;
    const unsigned int nb = flat_grid(work);
    {
        Prof pr(ctx, PGW_K_BYTESWAP);
        if (elem_bytes == 4)
            hipLaunchKernelGGL((k_byteswap<4>), dim3(nb), dim3(BLOCK), 0, ctx->stream, n16, n, (const uint4 *)src, (uint4 *)dst);
        else
            hipLaunchKernelGGL((k_byteswap<8>), dim3(nb), dim3(BLOCK), 0, ctx->stream, n16, n, (const uint4 *)src, (uint4 *)dst);
    }
    HIPCHK(ctx, hipGetLastError());
    return PGW_OK;
}

extern "C" int pgw_narrow_f64_f32(pgw_ctx *ctx, long long n, const double *src, void *dst, int big_endian) {
    NEED(ctx, n >= 0 && (n == 0 || (src && dst)), "bad argument");
    if (n == 0) return PGW_OK;
    NEED(ctx, ((uintptr_t)src % 8) == 0 && ((uintptr_t)dst % 4) == 0, "pointers must be element-aligned");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const bool al = ((uintptr_t)src % 16) == 0 && ((uintptr_t)dst % 8) == 0;
    const long long n2 = al ? n / 2 : 0;
    const unsigned int nb = flat_grid(n2 ? n2 : n);
    {
        Prof pr(ctx, PGW_K_BYTESWAP);
        if (big_endian) hipLaunchKernelGGL((k_narrow_f64_f32<true>), dim3(nb), dim3(BLOCK), 0, ctx->stream, n2, n, src, (unsigned int *)dst);
        else hipLaunchKernelGGL((k_narrow_f64_f32<false>), dim3(nb), dim3(BLOCK), 0, ctx->stream, n2, n, src, (unsigned int *)dst);
    }
    HIPCHK(ctx, hipGetLastError());
    return PGW_OK;
}

extern "C" int pgw_test_log(pgw_ctx *ctx, long long n, const double *in, double *out) {
    NEED(ctx, n >= 1 && in && out, "bad argument");
    hipLaunchKernelGGL(k_test_log, dim3(nblocks(n, 256)), dim3(256), 0, ctx->stream, n, in, out, 0);
    HIPCHK(ctx, hipGetLastError());
    return PGW_OK;
}

extern "C" int pgw_test_log_table(pgw_ctx *ctx, long long n, const double *in, double *out) {
    NEED(ctx, n >= 1 && in && out, "bad argument");
    hipLaunchKernelGGL(k_test_log, dim3(nblocks(n, 256)), dim3(256), 0, ctx->stream, n, in, out, 1);
    HIPCHK(ctx, hipGetLastError());
    return PGW_OK;
}

extern "C" int pgw_test_log_f3(pgw_ctx *ctx, long long n, const double *in, double *out) {
    NEED(ctx, n >= 1 && in && out, "bad argument");
    hipLaunchKernelGGL(k_test_log, dim3(nblocks(n, 256)), dim3(256), 0, ctx->stream, n, in, out, 2);
    HIPCHK(ctx, hipGetLastError());
    return PGW_OK;
}

extern "C" int pgw_test_log_dd(pgw_ctx *ctx, long long n, const double *in, double *out) {
    NEED(ctx, n >= 1 && in && out, "bad argument");
    hipLaunchKernelGGL(k_test_log, dim3(nblocks(n, 256)), dim3(256), 0, ctx->stream, n, in, out, 3);
    HIPCHK(ctx, hipGetLastError());
    return PGW_OK;
}

extern "C" int pgw_test_exp_finite(pgw_ctx *ctx, long long n, const double *in, double *out) {
    NEED(ctx, n >= 1 && in && out, "bad argument");
    hipLaunchKernelGGL(k_test_exp_finite, dim3(nblocks(n, 256)), dim3(256), 0, ctx->stream, n, in, out, 0);
    HIPCHK(ctx, hipGetLastError());
    return PGW_OK;
}

extern "C" int pgw_test_exp_reduced(pgw_ctx *ctx, long long n, const double *in, double *out) {
    NEED(ctx, n >= 1 && in && out, "bad argument");
    hipLaunchKernelGGL(k_test_exp_finite, dim3(nblocks(n, 256)), dim3(256), 0, ctx->stream, n, in, out, 1);
    HIPCHK(ctx, hipGetLastError());
    return PGW_OK;
}

// ------------------------------------------------------------------ regridding
// The bracket tables over n targets - pgw_regrid_bilinear: one axis per call, the other NULL; pgw_regrid_points: both.  Rows lie
// in [-1, nlat_s] (-1 / nlat_s: the pole rows), columns in [0, nlon_s); an entry whose `skip` flag is set is never read.
static int check_brackets(pgw_ctx *ctx, const char *caller, long long n, const int *skip, const int *lat_lo, const int *lat_hi,
                          const int *lon_lo, const int *lon_hi, int nlat_s, int nlon_s, int south_row, int north_row) {
    NEED_AS(ctx, caller, !lat_lo || (south_row < nlat_s && north_row < nlat_s), "bad pole row");
    for (long long g = 0; g < n; ++g) {
        if (skip[g]) continue;
        if (lon_lo) NEED_AS(ctx, caller, lon_lo[g] >= 0 && lon_lo[g] < nlon_s && lon_hi[g] >= 0 && lon_hi[g] < nlon_s, "lon index out of range");
        if (!lat_lo) continue;
        NEED_AS(ctx, caller, lat_lo[g] >= -1 && lat_lo[g] <= nlat_s && lat_hi[g] >= -1 && lat_hi[g] <= nlat_s, "lat index out of range");
        // a pole row is only there when its zonal mean is taken: k_zonal_mean_rows leaves the pole value of a negative row unwritten
        NEED_AS(ctx, caller, south_row >= 0 || (lat_lo[g] != -1 && lat_hi[g] != -1), "south-pole row in the tables but south_row < 0");
        NEED_AS(ctx, caller, north_row >= 0 || (lat_lo[g] != nlat_s && lat_hi[g] != nlat_s), "north-pole row in the tables but north_row < 0");
    }
    return PGW_OK;
}

// Host tables -> device workspace slot 3 as [double tables][pole: 2 * nfield doubles][int tables], each list back to back in the
// order given and every `*dev` set to where its table lies.  The host tables may be freed after the call.
template <typename T> struct HostTable { const T *host; size_t n; const T **dev; };
static int tables_to_slot3(pgw_ctx *ctx, std::initializer_list<HostTable<double>> dbl, std::initializer_list<HostTable<int>> ints,
                           long long nfield, double **dpole) {
    HIPCHK(ctx, hipSetDevice(ctx->device));
    size_t td = 0, ti = 0, at = 0;
    for (const auto &t : dbl) td += sizeof(double) * t.n;
    for (const auto &t : ints) ti += sizeof(int) * t.n;
    const size_t tp = sizeof(double) * 2 * (size_t)nfield;
    char *tab = nullptr;
    if (int rc = ws_get(ctx, 3, td + tp + ti + 64, (void **)&tab)) return rc;
    std::vector<char> h(td + ti);                              // the pole values are the device's own: not staged, tp apart there
    for (const auto &t : dbl) { memcpy(h.data() + at, t.host, sizeof(double) * t.n); *t.dev = (const double *)(tab + at); at += sizeof(double) * t.n; }
    for (const auto &t : ints) { memcpy(h.data() + at, t.host, sizeof(int) * t.n); *t.dev = (const int *)(tab + tp + at); at += sizeof(int) * t.n; }
    *dpole = (double *)(tab + td);
    HIPCHK(ctx, hipMemcpyAsync(tab, h.data(), td, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(tab + td + tp, h.data() + td, ti, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return PGW_OK;
}

// zonal means of the source rows next to the poles -> dpole [nfield][2]; nothing to do without a pole row
static void launch_pole_means(pgw_ctx *ctx, int dtype, long long nfield, int nlat_s, int nlon_s, const void *src, int south_row,
                              int north_row, double *dpole) {
    if (south_row >= 0 || north_row >= 0)
        with_type(dtype, [&](auto t_) {
            using T = decltype(t_);
            hipLaunchKernelGGL((k_zonal_mean_rows<T>), dim3(nblocks(nfield * 2 * 64, BLOCK)), dim3(BLOCK), 0, ctx->stream, nfield,
                               nlat_s, nlon_s, (const T *)src, south_row, north_row, dpole);
        });
}

// z-slices of a launch with blocks_xy blocks per slice: enough blocks to fill 256 CUs several times over even for few targets
static unsigned int z_slices(long long blocks_xy, long long nfield) {
    return (unsigned int)std::clamp((8192 + blocks_xy - 1) / blocks_xy, 1ll, nfield);
}

// The launch geometry of k_regrid for nfield planes onto an nlat_t x nlon_t mesh at `out` (elements of dtype_out)
struct RegridGrid {
    int W;
    unsigned int bx, gz, nb;
    bool fits;
    RegridGrid(pgw_ctx *ctx, long long nfield, int nlat_t, int nlon_t, const void *out, int dtype_out) {
        // two target longitudes per thread (one 16-B / 8-B store per plane) when the row length and the output alignment allow
        W = (nlon_t % 2 == 0 && ((uintptr_t)out % (2 * elem_size(dtype_out))) == 0 && !ctx->opt[PGW_OPT_FORCE_VEC1]) ? 2 : 1;
        bx = nblocks(nlon_t, BLOCK * W);
        const long long xy = (long long)bx * nlat_t;
        gz = z_slices(xy, nfield);
        // z-slices in multiples of 8 where there are planes for it: one XCD per slice group (k_regrid)
        if (nfield >= 8) gz = (gz + 7u) / 8u * 8u;
        if (gz > nfield) gz = (unsigned int)nfield;
        fits = xy * gz < (1ll << 31);
        nb = fits ? (unsigned int)(xy * gz) : 0u;
    }
};

static void launch_regrid(pgw_ctx *ctx, const RegridGrid &g, int dtype_src, int dtype_out, long long nfield, int nlat_s, int nlon_s,
                          int nlat_t, int nlon_t, const void *src, const RegridTables &tb, const double *dpole, void *out) {
    with_type(dtype_src, [&](auto t_) { with_type(dtype_out, [&](auto o_) { with_int<2>(g.W - 1, [&](auto w_) {
        using T = decltype(t_);
        using TOUT = decltype(o_);
        // 4 planes per step (2: 6 % slower, 8: the same)
        hipLaunchKernelGGL((k_regrid<T, 4, decltype(w_)::value + 1, TOUT>), dim3(g.nb), dim3(BLOCK), 0, ctx->stream, nfield, nlat_s,
                           nlon_s, nlat_t, nlon_t, g.bx, g.gz, (const T *)src, tb, dpole, (TOUT *)out);
    }); }); });
}

extern "C" int pgw_regrid_bilinear(pgw_ctx *ctx, int dtype, long long nfield, int nlat_s, int nlon_s, int nlat_t,
                                   int nlon_t, const void *src, const int *lat_lo, const int *lat_hi,
                                   const double *lat_dx, const double *lat_Dx, const int *lat_oob, const int *lon_lo,
                                   const int *lon_hi, const double *lon_dx, const double *lon_Dx, const int *lon_oob,
                                   int south_row, int north_row, void *out) {
    NEED(ctx, dtype == PGW_F32 || dtype == PGW_F64, "dtype must be PGW_F32 or PGW_F64");
    NEED(ctx, nfield >= 1 && nlat_s >= 2 && nlon_s >= 2 && nlat_t >= 1 && nlon_t >= 1, "bad shape");
    NEED(ctx, src && out && lat_lo && lat_hi && lat_dx && lat_Dx && lat_oob && lon_lo && lon_hi && lon_dx && lon_Dx && lon_oob,
         "null pointer");
    if (int rc = check_brackets(ctx, __func__, nlat_t, lat_oob, lat_lo, lat_hi, nullptr, nullptr, nlat_s, nlon_s, south_row, north_row)) return rc;
    if (int rc = check_brackets(ctx, __func__, nlon_t, lon_oob, nullptr, nullptr, lon_lo, lon_hi, nlat_s, nlon_s, south_row, north_row)) return rc;
    const size_t a = (size_t)nlat_t, o = (size_t)nlon_t;
    RegridTables tb;
    double *dpole;
    if (int rc = tables_to_slot3(ctx, {{lat_dx, a, &tb.lat_dx}, {lat_Dx, a, &tb.lat_Dx}, {lon_dx, o, &tb.lon_dx}, {lon_Dx, o, &tb.lon_Dx}},
                              {{lat_lo, a, &tb.lat_lo}, {lat_hi, a, &tb.lat_hi}, {lat_oob, a, &tb.lat_oob},
                               {lon_lo, o, &tb.lon_lo}, {lon_hi, o, &tb.lon_hi}, {lon_oob, o, &tb.lon_oob}}, nfield, &dpole))
        return rc;
    {
        Prof pr(ctx, PGW_K_REGRID);
        launch_pole_means(ctx, dtype, nfield, nlat_s, nlon_s, src, south_row, north_row, dpole);
        const RegridGrid g(ctx, nfield, nlat_t, nlon_t, out, dtype);
        NEED(ctx, g.fits, "regrid: too many blocks");
        launch_regrid(ctx, g, dtype, dtype, nfield, nlat_s, nlon_s, nlat_t, nlon_t, src, tb, dpole, out);
    }
    HIPCHK(ctx, hipGetLastError());
    return PGW_OK;
}

// A regrid plan: the ten tables of one (source grid, target mesh) pair resident on the device, with the pole scratch of up
// to max_nfield planes behind them - what pgw_regrid_bilinear lays into workspace slot 3 on every call, held once.
struct pgw_regrid_plan {
    int nlat_s, nlon_s, nlat_t, nlon_t, south_row, north_row;
    long long max_nfield;
    RegridTables tb;
    double *dpole;
    char *mem;                                                 // one allocation: [double tables][pole][int tables]
};

extern "C" int pgw_regrid_plan_create(pgw_ctx *ctx, int nlat_s, int nlon_s, int nlat_t, int nlon_t, const int *lat_lo,
                                      const int *lat_hi, const double *lat_dx, const double *lat_Dx, const int *lat_oob,
                                      const int *lon_lo, const int *lon_hi, const double *lon_dx, const double *lon_Dx,
                                      const int *lon_oob, int south_row, int north_row, long long max_nfield,
                                      pgw_regrid_plan **plan) {
    NEED(ctx, plan, "null pointer");
    *plan = nullptr;
    NEED(ctx, max_nfield >= 1 && max_nfield < (1ll << 40) && nlat_s >= 2 && nlon_s >= 2 && nlat_t >= 1 && nlon_t >= 1, "bad shape");
    NEED(ctx, lat_lo && lat_hi && lat_dx && lat_Dx && lat_oob && lon_lo && lon_hi && lon_dx && lon_Dx && lon_oob, "null pointer");
    if (int rc = check_brackets(ctx, __func__, nlat_t, lat_oob, lat_lo, lat_hi, nullptr, nullptr, nlat_s, nlon_s, south_row, north_row)) return rc;
    if (int rc = check_brackets(ctx, __func__, nlon_t, lon_oob, nullptr, nullptr, lon_lo, lon_hi, nlat_s, nlon_s, south_row, north_row)) return rc;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const size_t a = (size_t)nlat_t, o = (size_t)nlon_t;
    const size_t td = sizeof(double) * 2 * (a + o), tp = sizeof(double) * 2 * (size_t)max_nfield, ti = sizeof(int) * 3 * (a + o);
    std::vector<char> h(td + ti);
    pgw_regrid_plan *p = new pgw_regrid_plan{nlat_s, nlon_s, nlat_t, nlon_t, south_row, north_row, max_nfield, {}, nullptr, nullptr};
    const hipError_t e = hipMalloc((void **)&p->mem, td + tp + ti);
    if (e != hipSuccess) {
        (void)hipGetLastError();                               // as pgw_malloc: an allocation that does not fit is an answer
        delete p;
        return fail(ctx, PGW_ERR_HIP, "hipMalloc(%zu bytes) failed: %s", td + tp + ti, hipGetErrorString(e));
    }
    size_t at = 0;
    auto put = [&](const auto *host, size_t n, auto **dev, size_t gap) {
        memcpy(h.data() + at, host, sizeof(*host) * n);
        *dev = (std::remove_reference_t<decltype(*dev)>)(p->mem + gap + at);
        at += sizeof(*host) * n;
    };
    put(lat_dx, a, &p->tb.lat_dx, 0); put(lat_Dx, a, &p->tb.lat_Dx, 0); put(lon_dx, o, &p->tb.lon_dx, 0); put(lon_Dx, o, &p->tb.lon_Dx, 0);
    p->dpole = (double *)(p->mem + td);
    put(lat_lo, a, &p->tb.lat_lo, tp); put(lat_hi, a, &p->tb.lat_hi, tp); put(lat_oob, a, &p->tb.lat_oob, tp);
    put(lon_lo, o, &p->tb.lon_lo, tp); put(lon_hi, o, &p->tb.lon_hi, tp); put(lon_oob, o, &p->tb.lon_oob, tp);
    hipError_t c = hipMemcpyAsync(p->mem, h.data(), td, hipMemcpyHostToDevice, ctx->stream);
    if (c == hipSuccess) c = hipMemcpyAsync(p->mem + td + tp, h.data() + td, ti, hipMemcpyHostToDevice, ctx->stream);
    if (c == hipSuccess) c = hipStreamSynchronize(ctx->stream);        // once per plan: the host tables may be freed after the call
    if (c != hipSuccess) {
        (void)hipFree(p->mem);
        delete p;
        return fail(ctx, PGW_ERR_HIP, "upload of the regrid tables failed: %s", hipGetErrorString(c));
    }
    *plan = p;
    return PGW_OK;
}

extern "C" int pgw_regrid_plan_apply(pgw_ctx *ctx, const pgw_regrid_plan *plan, int dtype_src, int dtype_out, long long nfield,
                                     const void *src, void *out) {
    NEED(ctx, plan, "null plan");
    NEED(ctx, (dtype_src == PGW_F32 || dtype_src == PGW_F64) && (dtype_out == PGW_F32 || dtype_out == PGW_F64),
         "dtypes must be PGW_F32 or PGW_F64");
    NEED(ctx, nfield >= 1 && nfield <= plan->max_nfield, "nfield must be in [1, max_nfield of the plan]");
    NEED(ctx, src && out, "null pointer");
    NEED(ctx, ((uintptr_t)src % elem_size(dtype_src)) == 0 && ((uintptr_t)out % elem_size(dtype_out)) == 0, "pointers must be element-aligned");
    const RegridGrid g(ctx, nfield, plan->nlat_t, plan->nlon_t, out, dtype_out);
    NEED(ctx, g.fits, "regrid: too many blocks");
    {
        Prof pr(ctx, PGW_K_REGRID);
        launch_pole_means(ctx, dtype_src, nfield, plan->nlat_s, plan->nlon_s, src, plan->south_row, plan->north_row, plan->dpole);
        launch_regrid(ctx, g, dtype_src, dtype_out, nfield, plan->nlat_s, plan->nlon_s, plan->nlat_t, plan->nlon_t, src, plan->tb,
                      plan->dpole, out);
    }
    HIPCHK(ctx, hipGetLastError());
    return PGW_OK;
}

extern "C" int pgw_regrid_plan_destroy(pgw_ctx *ctx, pgw_regrid_plan *plan) {
    if (!plan) return PGW_OK;
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));            // no launch may still read the tables
    HIPCHK(ctx, hipFree(plan->mem));
    delete plan;
    return PGW_OK;
}

// The shapes and the nine host tables of a point-wise call or plan (nfield: the planes of the call, max_nfield of a plan)
static int check_point_shapes(pgw_ctx *ctx, const char *caller, long long nfield, int nlat_s, int nlon_s, long long ntarg,
                              const int *lat_lo, const int *lat_hi, const double *lat_dx, const double *lat_Dx, const int *lon_lo,
                              const int *lon_hi, const double *lon_dx, const double *lon_Dx, const int *oob) {
    NEED_AS(ctx, caller, nfield >= 1 && ntarg >= 1 && ntarg < (1ll << 29), "nfield >= 1 and ntarg in [1, 2^29)");
    NEED_AS(ctx, caller, nlat_s >= 2 && nlon_s >= 2 && (long long)nlat_s * nlon_s < (1ll << 30), "source grid must be at least 2 x 2 (and below 2^30 nodes)");
    NEED_AS(ctx, caller, lat_lo && lat_hi && lat_dx && lat_Dx && lon_lo && lon_hi && lon_dx && lon_Dx && oob, "null pointer");
    return PGW_OK;
}

// What the point-wise entries check and upload before they launch, under the name of the entry: dtype, shapes, the `narrays`
// device arrays (non-null, element-aligned), the nine host tables and their brackets; then the tables into slot 3 with room
// for the pole values of `pole_planes` planes behind them.
static int point_tables(pgw_ctx *ctx, const char *caller, int dtype, long long nfield, int nlat_s, int nlon_s, long long ntarg,
                        const void *const *arrays, int narrays, const int *lat_lo, const int *lat_hi, const double *lat_dx,
                        const double *lat_Dx, const int *lon_lo, const int *lon_hi, const double *lon_dx, const double *lon_Dx,
                        const int *oob, int south_row, int north_row, long long pole_planes, PointTables *tb, double **dpole) {
    NEED_AS(ctx, caller, dtype == PGW_F32 || dtype == PGW_F64, "dtype must be PGW_F32 or PGW_F64");
    if (int rc = check_point_shapes(ctx, caller, nfield, nlat_s, nlon_s, ntarg, lat_lo, lat_hi, lat_dx, lat_Dx, lon_lo, lon_hi, lon_dx, lon_Dx, oob)) return rc;
    for (int k = 0; k < narrays; ++k) {
        NEED_AS(ctx, caller, arrays[k], "null pointer");
        NEED_AS(ctx, caller, ((uintptr_t)arrays[k] % elem_size(dtype)) == 0, "pointers must be element-aligned");
    }
    if (int rc = check_brackets(ctx, caller, ntarg, oob, lat_lo, lat_hi, lon_lo, lon_hi, nlat_s, nlon_s, south_row, north_row)) return rc;
    const size_t n = (size_t)ntarg;
    return tables_to_slot3(ctx, {{lat_dx, n, &tb->lat_dx}, {lat_Dx, n, &tb->lat_Dx}, {lon_dx, n, &tb->lon_dx}, {lon_Dx, n, &tb->lon_Dx}},
                           {{lat_lo, n, &tb->lat_lo}, {lat_hi, n, &tb->lat_hi}, {lon_lo, n, &tb->lon_lo}, {lon_hi, n, &tb->lon_hi}, {oob, n, &tb->oob}},
                           pole_planes, dpole);
}

// The pole means and k_regrid_points for nfield planes onto ntarg targets, timed under PGW_K_REGRID: one target per thread
static void launch_points(pgw_ctx *ctx, int dtype_src, int dtype_out, long long nfield, int nlat_s, int nlon_s, long long ntarg,
                          const void *src, const PointTables &tb, int south_row, int north_row, double *dpole, void *out) {
    const unsigned int bx = nblocks(ntarg, BLOCK);
    const unsigned int gz = std::min(z_slices(bx, nfield), 65535u);          // blockIdx.y
    Prof pr(ctx, PGW_K_REGRID);
    launch_pole_means(ctx, dtype_src, nfield, nlat_s, nlon_s, src, south_row, north_row, dpole);
    with_type(dtype_src, [&](auto t_) { with_type(dtype_out, [&](auto o_) {
        using T = decltype(t_);
        using TOUT = decltype(o_);
        hipLaunchKernelGGL((k_regrid_points<T, TOUT>), dim3(bx, gz), dim3(BLOCK), 0, ctx->stream, nfield, nlat_s, nlon_s, ntarg, gz,
                           (const T *)src, tb, dpole, (TOUT *)out);
    }); });
}

// The same for both wind components and the rotation behind them (k_regrid_points_wind); dpole takes [2][nfield][2]
static void launch_points_wind(pgw_ctx *ctx, int dtype_src, int dtype_out, long long nfield, int nlat_s, int nlon_s, long long ntarg,
                               const void *src_u, const void *src_v, const PointTables &tb, int south_row, int north_row,
                               double *dpole, const double *cos, const double *sin, void *u_out, void *v_out) {
    const unsigned int bx = nblocks(ntarg, BLOCK);
    const unsigned int gz = std::min(z_slices(bx, nfield), 65535u);          // blockIdx.y
    double *dpole_v = dpole + 2 * nfield;                     // [nfield][2] each
    Prof pr(ctx, PGW_K_REGRID);
    launch_pole_means(ctx, dtype_src, nfield, nlat_s, nlon_s, src_u, south_row, north_row, dpole);
    launch_pole_means(ctx, dtype_src, nfield, nlat_s, nlon_s, src_v, south_row, north_row, dpole_v);
    with_type(dtype_src, [&](auto t_) { with_type(dtype_out, [&](auto o_) {
        using T = decltype(t_);
        using TOUT = decltype(o_);
        hipLaunchKernelGGL((k_regrid_points_wind<T, TOUT>), dim3(bx, gz), dim3(BLOCK), 0, ctx->stream, nfield, nlat_s, nlon_s, ntarg,
                           gz, (const T *)src_u, (const T *)src_v, tb, dpole, dpole_v, cos, sin, (TOUT *)u_out, (TOUT *)v_out);
    }); });
}

// regrid_lat_lon, xarray branch with point-wise targets (functions.py:812-893 with 2-D targ_lat / targ_lon)
extern "C" int pgw_regrid_points(pgw_ctx *ctx, int dtype, long long nfield, int nlat_s, int nlon_s, long long ntarg, const void *src,
                                 const int *lat_lo, const int *lat_hi, const double *lat_dx, const double *lat_Dx, const int *lon_lo,
                                 const int *lon_hi, const double *lon_dx, const double *lon_Dx, const int *oob, int south_row,
                                 int north_row, void *out) {
    const void *arrays[] = {src, out};
    PointTables tb;
    double *dpole;
    if (int rc = point_tables(ctx, __func__, dtype, nfield, nlat_s, nlon_s, ntarg, arrays, 2, lat_lo, lat_hi, lat_dx, lat_Dx, lon_lo, lon_hi,
                              lon_dx, lon_Dx, oob, south_row, north_row, nfield, &tb, &dpole))
        return rc;
    launch_points(ctx, dtype, dtype, nfield, nlat_s, nlon_s, ntarg, src, tb, south_row, north_row, dpole, out);
    HIPCHK(ctx, hipGetLastError());
    return PGW_OK;
}

// ------------------------------------------------------------------ winds on a rotated-pole target grid
extern "C" int pgw_wind_rotation(pgw_ctx *ctx, long long n, const double *lat, const double *lon, double pole_lat, double pole_lon,
                                 double *cos_out, double *sin_out) {
    NEED(ctx, n >= 1 && n < (1ll << 31) && lat && lon && cos_out && sin_out, "n must be in [1, 2^31), the pointers not null");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    {
        Prof pr(ctx, PGW_K_REGRID);
        hipLaunchKernelGGL(k_wind_rotation, dim3(nblocks(n, BLOCK)), dim3(BLOCK), 0, ctx->stream, n, lat, lon, pole_lat, pole_lon, cos_out,
                           sin_out);
    }
    HIPCHK(ctx, hipGetLastError());
    return PGW_OK;
}

// planes per z-slice of k_rotate_pair, where there are that many: the 16 bytes of c and s a lane loads per target are then at
// most a third of what its planes move (float32: 8 bytes in and 8 out per target and plane, float64 twice that)
static const long long ROTATE_MIN_PLANES = 3;

extern "C" int pgw_rotate_pair(pgw_ctx *ctx, int dtype, long long nfield, long long n, const void *u, const void *v, const double *cos,
                               const double *sin, int inverse, void *u_out, void *v_out) {
    NEED(ctx, dtype == PGW_F32 || dtype == PGW_F64, "dtype must be PGW_F32 or PGW_F64");
    NEED(ctx, nfield >= 1 && nfield < (1ll << 40) && n >= 1 && n < (1ll << 31), "nfield >= 1 and n in [1, 2^31)");
    NEED(ctx, u && v && cos && sin && u_out && v_out, "null pointer");
    const size_t es = elem_size(dtype);
    NEED(ctx, (uintptr_t)u % es == 0 && (uintptr_t)v % es == 0 && (uintptr_t)u_out % es == 0 && (uintptr_t)v_out % es == 0 &&
                  (uintptr_t)cos % 8 == 0 && (uintptr_t)sin % 8 == 0, "pointers must be element-aligned");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    // 16 bytes of T per lane and access (planes start n elements apart: n must be a multiple of it), or one element
    const int full = dtype == PGW_F64 ? 2 : 4;
    const int vec = pick_vec(ctx, dtype, n, {u, v, cos, sin, u_out, v_out}) == full ? full : 1;
    const unsigned int bx = nblocks(n / vec, BLOCK);
    const long long most = (nfield + ROTATE_MIN_PLANES - 1) / ROTATE_MIN_PLANES;
    const unsigned int gz = (unsigned int)std::min({(long long)z_slices(bx, nfield), most, 65535ll});      // blockIdx.y
    {
        Prof pr(ctx, PGW_K_REGRID);
        with_type(dtype, [&](auto t_) { with_int<2>(vec > 1, [&](auto wide_) {
            using T = decltype(t_);
            constexpr int V = decltype(wide_)::value ? 16 / (int)sizeof(T) : 1;
            hipLaunchKernelGGL((k_rotate_pair<T, V>), dim3(bx, gz), dim3(BLOCK), 0, ctx->stream, nfield, n, gz, (const T *)u,
                               (const T *)v, cos, sin, inverse, (T *)u_out, (T *)v_out);
        }); });
    }
    HIPCHK(ctx, hipGetLastError());
    return PGW_OK;
}

// pgw_regrid_points on ua and va together, rotated onto the targets' grid-relative directions in the same launch
extern "C" int pgw_regrid_points_wind(pgw_ctx *ctx, int dtype, long long nfield, int nlat_s, int nlon_s, long long ntarg,
                                      const void *src_u, const void *src_v, const int *lat_lo, const int *lat_hi, const double *lat_dx,
                                      const double *lat_Dx, const int *lon_lo, const int *lon_hi, const double *lon_dx,
                                      const double *lon_Dx, const int *oob, int south_row, int north_row, const double *cos,
                                      const double *sin, void *u_out, void *v_out) {
    NEED(ctx, cos && sin && (uintptr_t)cos % 8 == 0 && (uintptr_t)sin % 8 == 0, "cos / sin: null or misaligned pointer");
    NEED(ctx, nfield < (1ll << 40), "nfield must be below 2^40");
    const void *arrays[] = {src_u, src_v, u_out, v_out};
    PointTables tb;
    double *dpole;
    if (int rc = point_tables(ctx, __func__, dtype, nfield, nlat_s, nlon_s, ntarg, arrays, 4, lat_lo, lat_hi, lat_dx, lat_Dx, lon_lo, lon_hi,
                              lon_dx, lon_Dx, oob, south_row, north_row, 2 * nfield, &tb, &dpole))
        return rc;
    launch_points_wind(ctx, dtype, dtype, nfield, nlat_s, nlon_s, ntarg, src_u, src_v, tb, south_row, north_row, dpole, cos, sin, u_out,
                       v_out);
    HIPCHK(ctx, hipGetLastError());
    return PGW_OK;
}

// A points plan: the nine tables of one (source grid, target list) pair resident on the device, the targets' cos / sin behind
// them where the plan rotates, and the pole scratch of up to 2 * max_nfield planes (u and v) - what the point-wise entries lay
// into workspace slot 3 on every call, held once.
struct pgw_points_plan {
    int nlat_s, nlon_s, south_row, north_row;
    long long ntarg, max_nfield;
    PointTables tb;
    const double *cs, *sn;                                     // null: the plan cannot rotate
    double *dpole;
    char *mem;                                                 // one allocation: [double tables][cos][sin][pole][int tables]
};

extern "C" int pgw_points_plan_create(pgw_ctx *ctx, int nlat_s, int nlon_s, long long ntarg, const int *lat_lo, const int *lat_hi,
                                      const double *lat_dx, const double *lat_Dx, const int *lon_lo, const int *lon_hi,
                                      const double *lon_dx, const double *lon_Dx, const int *oob, int south_row, int north_row,
                                      long long max_nfield, const double *cos, const double *sin, pgw_points_plan **plan) {
    NEED(ctx, plan, "null pointer");
    *plan = nullptr;
    NEED(ctx, max_nfield < (1ll << 40), "max_nfield must be below 2^40");
    if (int rc = check_point_shapes(ctx, __func__, max_nfield, nlat_s, nlon_s, ntarg, lat_lo, lat_hi, lat_dx, lat_Dx, lon_lo, lon_hi, lon_dx, lon_Dx, oob)) return rc;
    NEED(ctx, (cos == nullptr) == (sin == nullptr), "cos and sin: both or neither");
    NEED(ctx, (uintptr_t)cos % 8 == 0 && (uintptr_t)sin % 8 == 0, "cos / sin: misaligned pointer");
    if (int rc = check_brackets(ctx, __func__, ntarg, oob, lat_lo, lat_hi, lon_lo, lon_hi, nlat_s, nlon_s, south_row, north_row)) return rc;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const size_t n = (size_t)ntarg;
    const size_t td = sizeof(double) * 4 * n, tr = cos ? sizeof(double) * 2 * n : 0, tp = sizeof(double) * 4 * (size_t)max_nfield,
                 ti = sizeof(int) * 5 * n;
    std::vector<char> h(td + ti);
    pgw_points_plan *p = new pgw_points_plan{nlat_s, nlon_s, south_row, north_row, ntarg, max_nfield, {}, nullptr, nullptr, nullptr, nullptr};
    const hipError_t e = hipMalloc((void **)&p->mem, td + tr + tp + ti);
    if (e != hipSuccess) {
        (void)hipGetLastError();                               // as pgw_malloc: an allocation that does not fit is an answer
        delete p;
        return fail(ctx, PGW_ERR_HIP, "hipMalloc(%zu bytes) failed: %s", td + tr + tp + ti, hipGetErrorString(e));
    }
    size_t at = 0;
    auto put = [&](const auto *host, auto **dev, size_t gap) {
        memcpy(h.data() + at, host, sizeof(*host) * n);
        *dev = (std::remove_reference_t<decltype(*dev)>)(p->mem + gap + at);
        at += sizeof(*host) * n;
    };
    put(lat_dx, &p->tb.lat_dx, 0); put(lat_Dx, &p->tb.lat_Dx, 0); put(lon_dx, &p->tb.lon_dx, 0); put(lon_Dx, &p->tb.lon_Dx, 0);
    p->dpole = (double *)(p->mem + td + tr);
    put(lat_lo, &p->tb.lat_lo, tr + tp); put(lat_hi, &p->tb.lat_hi, tr + tp); put(lon_lo, &p->tb.lon_lo, tr + tp);
    put(lon_hi, &p->tb.lon_hi, tr + tp); put(oob, &p->tb.oob, tr + tp);
    hipError_t c = hipMemcpyAsync(p->mem, h.data(), td, hipMemcpyHostToDevice, ctx->stream);
    if (c == hipSuccess) c = hipMemcpyAsync(p->mem + td + tr + tp, h.data() + td, ti, hipMemcpyHostToDevice, ctx->stream);
    if (cos) {
        p->cs = (const double *)(p->mem + td);
        p->sn = p->cs + n;
        if (c == hipSuccess) c = hipMemcpyAsync((void *)p->cs, cos, sizeof(double) * n, hipMemcpyDeviceToDevice, ctx->stream);
        if (c == hipSuccess) c = hipMemcpyAsync((void *)p->sn, sin, sizeof(double) * n, hipMemcpyDeviceToDevice, ctx->stream);
    }
    if (c == hipSuccess) c = hipStreamSynchronize(ctx->stream);        // once per plan: the host tables may be freed after the call
    if (c != hipSuccess) {
        (void)hipFree(p->mem);
        delete p;
        return fail(ctx, PGW_ERR_HIP, "upload of the point tables failed: %s", hipGetErrorString(c));
    }
    *plan = p;
    return PGW_OK;
}

// What both apply entries check before they launch: the plan, the dtype tags, nfield and the `narrays` device arrays - the
// first half of them sources (dtype_src), the second half outputs (dtype_out)
static int check_points_apply(pgw_ctx *ctx, const char *caller, const pgw_points_plan *plan, int dtype_src, int dtype_out, long long nfield,
                              const void *const *arrays, int narrays) {
    NEED_AS(ctx, caller, plan, "null plan");
    NEED_AS(ctx, caller, (dtype_src == PGW_F32 || dtype_src == PGW_F64) && (dtype_out == PGW_F32 || dtype_out == PGW_F64),
            "dtypes must be PGW_F32 or PGW_F64");
    NEED_AS(ctx, caller, nfield >= 1 && nfield <= plan->max_nfield, "nfield must be in [1, max_nfield of the plan]");
    for (int k = 0; k < narrays; ++k) {
        NEED_AS(ctx, caller, arrays[k], "null pointer");
        NEED_AS(ctx, caller, ((uintptr_t)arrays[k] % elem_size(k < narrays / 2 ? dtype_src : dtype_out)) == 0, "pointers must be element-aligned");
    }
    return PGW_OK;
}

extern "C" int pgw_points_plan_apply(pgw_ctx *ctx, const pgw_points_plan *plan, int dtype_src, int dtype_out, long long nfield,
                                     const void *src, void *out) {
    const void *arrays[] = {src, out};
    if (int rc = check_points_apply(ctx, __func__, plan, dtype_src, dtype_out, nfield, arrays, 2)) return rc;
    launch_points(ctx, dtype_src, dtype_out, nfield, plan->nlat_s, plan->nlon_s, plan->ntarg, src, plan->tb, plan->south_row,
                  plan->north_row, plan->dpole, out);
    HIPCHK(ctx, hipGetLastError());
    return PGW_OK;
}

extern "C" int pgw_points_plan_apply_wind(pgw_ctx *ctx, const pgw_points_plan *plan, int dtype_src, int dtype_out, long long nfield,
                                          const void *src_u, const void *src_v, void *u_out, void *v_out) {
    const void *arrays[] = {src_u, src_v, u_out, v_out};
    if (int rc = check_points_apply(ctx, __func__, plan, dtype_src, dtype_out, nfield, arrays, 4)) return rc;
    NEED(ctx, plan->cs, "the plan was made without cos / sin and cannot rotate");
    launch_points_wind(ctx, dtype_src, dtype_out, nfield, plan->nlat_s, plan->nlon_s, plan->ntarg, src_u, src_v, plan->tb,
                       plan->south_row, plan->north_row, plan->dpole, plan->cs, plan->sn, u_out, v_out);
    HIPCHK(ctx, hipGetLastError());
    return PGW_OK;
}

extern "C" int pgw_points_plan_destroy(pgw_ctx *ctx, pgw_points_plan *plan) {
    if (!plan) return PGW_OK;
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));            // no launch may still read the tables
    HIPCHK(ctx, hipFree(plan->mem));
    delete plan;
    return PGW_OK;
}

// regrid_lat_lon, xESMF branch (functions.py:797-810): locate once per grid pair ...
extern "C" int pgw_bilinear_locate(pgw_ctx *ctx, long long ntarg, const double *P, int ny, int nx, int periodic, const double *X,
                                   int nb, const int *bucket_start, const int *bucket_cells, int *idx, double *w,
                                   long long *n_unmapped) {
    NEED(ctx, ntarg >= 1 && ntarg < (1ll << 29), "ntarg must be in [1, 2^29)");
    NEED(ctx, ny >= 2 && nx >= 2 && (long long)ny * nx < (1ll << 30), "source grid must be at least 2 x 2 (and below 2^30 nodes)");
    NEED(ctx, nb >= 1 && nb <= 512, "nb must be in [1, 512]");
    NEED(ctx, P && X && bucket_start && bucket_cells && idx && w && n_unmapped, "null pointer");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    void *ws = nullptr;
    int rc = ws_get(ctx, 3, 64, &ws);
    if (rc) return rc;
    unsigned int *d_count = (unsigned int *)ws;
    HIPCHK(ctx, hipMemsetAsync(d_count, 0, sizeof(unsigned int), ctx->stream));
    {
        Prof pr(ctx, PGW_K_CELL_LOCATE);
        hipLaunchKernelGGL(k_cell_locate, dim3(nblocks(ntarg, BLOCK)), dim3(BLOCK), 0, ctx->stream, ntarg, P, ny, nx, periodic ? 1 : 0, X,
                           nb, bucket_start, bucket_cells, idx, w, d_count);
    }
    HIPCHK(ctx, hipGetLastError());
    unsigned int h_count = 0;
    HIPCHK(ctx, hipMemcpyAsync(&h_count, d_count, sizeof(unsigned int), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    *n_unmapped = (long long)h_count;
    return PGW_OK;
}

// ... and apply to every plane (regridder(ds_in[var_name]), functions.py:802)
extern "C" int pgw_regrid_sparse(pgw_ctx *ctx, int dtype, long long nfield, int ny, int nx, long long ntarg, const void *src,
                                 const int *idx, const double *w, int unmapped_nan, void *out) {
    NEED(ctx, dtype == PGW_F32 || dtype == PGW_F64, "dtype must be PGW_F32 or PGW_F64");
    NEED(ctx, nfield >= 1 && ntarg >= 1 && ntarg < (1ll << 29), "nfield >= 1 and ntarg in [1, 2^29)");
    NEED(ctx, ny >= 2 && nx >= 2 && (long long)ny * nx < (1ll << 30), "source grid must be at least 2 x 2 (and below 2^30 nodes)");
    NEED(ctx, src && idx && w && out, "null pointer");
    NEED(ctx, ((uintptr_t)src % elem_size(dtype)) == 0 && ((uintptr_t)out % elem_size(dtype)) == 0, "pointers must be element-aligned");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    void *ws = nullptr;
    if (int rc = ws_get(ctx, 3, 64 + sizeof(double) * 2 * (size_t)nfield, &ws)) return rc;
    double *dpole = (double *)((char *)ws + 64);
    // 16 bytes of a plane per thread when the plane length and the output's alignment allow
    const int wide = (int)(16 / elem_size(dtype));
    const int W = (ntarg % wide == 0 && aligned16(out) && !ctx->opt[PGW_OPT_FORCE_VEC1]) ? wide : 1;
    const unsigned int bx = nblocks(ntarg, BLOCK * W);
    const unsigned int gz = std::min(z_slices(bx, nfield), 65535u);          // blockIdx.y
    {
        Prof pr(ctx, PGW_K_REGRID_SPARSE);
        with_type(dtype, [&](auto t_) {
            using T = decltype(t_);
            hipLaunchKernelGGL((k_row_mean_plain<T>), dim3(nblocks(nfield * 2 * 64, BLOCK)), dim3(BLOCK), 0, ctx->stream, nfield, ny, nx,
                               (const T *)src, dpole);
            auto form = [&](auto w_) {
                hipLaunchKernelGGL((k_regrid_sparse<T, decltype(w_)::value>), dim3(bx, gz), dim3(BLOCK), 0, ctx->stream, nfield,
                                   (long long)ny * nx, ntarg, gz, (const T *)src, idx, w, dpole, unmapped_nan ? 1 : 0,
                                   ctx->opt[PGW_OPT_SPARSE_DIRECT] ? 1 : 0, (T *)out);
            };
            if (W == 1) form(int_c<1>()); else form(int_c<(int)(16 / sizeof(T))>());
        });
    }
    HIPCHK(ctx, hipGetLastError());
    return PGW_OK;
}

// ... on ua and va of a rotated-pole source together: turned to geographic in front of the weights, onto a rotated target's
// directions behind them (k_row_mean_plain_wind, k_regrid_sparse_wind)
extern "C" int pgw_regrid_sparse_wind(pgw_ctx *ctx, int dtype, long long nfield, int ny, int nx, long long ntarg, const void *src_u,
                                      const void *src_v, const double *src_cos, const double *src_sin, const int *idx, const double *w,
                                      int unmapped_nan, const double *targ_cos, const double *targ_sin, void *u_out, void *v_out) {
    NEED(ctx, dtype == PGW_F32 || dtype == PGW_F64, "dtype must be PGW_F32 or PGW_F64");
    NEED(ctx, nfield >= 1 && nfield < (1ll << 30) && ntarg >= 1 && ntarg < (1ll << 29), "nfield in [1, 2^30) and ntarg in [1, 2^29)");
    NEED(ctx, ny >= 2 && nx >= 2 && (long long)ny * nx < (1ll << 30), "source grid must be at least 2 x 2 (and below 2^30 nodes)");
    NEED(ctx, src_u && src_v && idx && w && u_out && v_out, "null pointer");
    NEED(ctx, (src_cos == nullptr) == (src_sin == nullptr), "src_cos and src_sin: both or neither");
    NEED(ctx, (targ_cos == nullptr) == (targ_sin == nullptr), "targ_cos and targ_sin: both or neither");
    const size_t es = elem_size(dtype);
    NEED(ctx, (uintptr_t)src_u % es == 0 && (uintptr_t)src_v % es == 0 && (uintptr_t)u_out % es == 0 && (uintptr_t)v_out % es == 0 &&
                  (uintptr_t)src_cos % 8 == 0 && (uintptr_t)src_sin % 8 == 0 && (uintptr_t)targ_cos % 8 == 0 &&
                  (uintptr_t)targ_sin % 8 == 0 && (uintptr_t)idx % 4 == 0 && (uintptr_t)w % 8 == 0, "pointers must be element-aligned");
    // the outputs are written with streaming stores while other blocks still read: they may overlap nothing the kernels read
    const size_t nsrc = (size_t)ny * nx, nt = (size_t)ntarg, out_bytes = (size_t)nfield * nt * es;
    const struct { const void *p; size_t bytes; } reads[] = {
        {src_u, (size_t)nfield * nsrc * es}, {src_v, (size_t)nfield * nsrc * es}, {src_cos, nsrc * 8}, {src_sin, nsrc * 8},
        {idx, nt * 4 * sizeof(int)}, {w, nt * 4 * 8}, {targ_cos, nt * 8}, {targ_sin, nt * 8}};
    auto overlap = [](const void *a, size_t na, const void *b, size_t nb) {
        return a && b && (uintptr_t)a < (uintptr_t)b + nb && (uintptr_t)b < (uintptr_t)a + na;
    };
    for (const auto &r : reads)
        NEED(ctx, !overlap(u_out, out_bytes, r.p, r.bytes) && !overlap(v_out, out_bytes, r.p, r.bytes), "an output aliases an input");
    NEED(ctx, !overlap(u_out, out_bytes, v_out, out_bytes), "u_out and v_out alias each other");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    void *ws = nullptr;
    if (int rc = ws_get(ctx, 3, 64 + sizeof(double) * 4 * (size_t)nfield, &ws)) return rc;
    double *dpole_u = (double *)((char *)ws + 64), *dpole_v = dpole_u + 2 * nfield;      // [nfield][2] each
    // two targets per thread when the plane length and the outputs' alignment allow: 16-byte stores of float64, 8-byte ones of
    // float32, whose four-wide form would need 310 registers (one wave per SIMD) for the entries' idx, w, cos and sin
    const int wide = 2;
    const int W = (ntarg % wide == 0 && aligned16(u_out) && aligned16(v_out) && !ctx->opt[PGW_OPT_FORCE_VEC1]) ? wide : 1;
    const unsigned int bx = nblocks(ntarg, BLOCK * W);
    const unsigned int gz = std::min(z_slices(bx, nfield), 65535u);          // blockIdx.y
    {
        Prof pr(ctx, PGW_K_REGRID_SPARSE);
        with_type(dtype, [&](auto t_) {
            using T = decltype(t_);
            hipLaunchKernelGGL((k_row_mean_plain_wind<T>), dim3(nblocks(nfield * 2 * 64, BLOCK)), dim3(BLOCK), 0, ctx->stream, nfield, ny,
                               nx, (const T *)src_u, (const T *)src_v, src_cos, src_sin, dpole_u, dpole_v);
            auto form = [&](auto w_) {
                hipLaunchKernelGGL((k_regrid_sparse_wind<T, decltype(w_)::value>), dim3(bx, gz), dim3(BLOCK), 0, ctx->stream, nfield,
                                   (long long)ny * nx, ntarg, gz, (const T *)src_u, (const T *)src_v, src_cos, src_sin, idx, w, dpole_u,
                                   dpole_v, unmapped_nan ? 1 : 0, ctx->opt[PGW_OPT_SPARSE_DIRECT] ? 1 : 0, targ_cos, targ_sin,
                                   (T *)u_out, (T *)v_out);
            };
            if (W == 1) form(int_c<1>()); else form(int_c<2>());
        });
    }
    HIPCHK(ctx, hipGetLastError());
    return PGW_OK;
}

// ------------------------------------------------------------------ surface riders
extern "C" int pgw_integrate_tos(pgw_ctx *ctx, int dtype, long long n, const void *tos, const void *ts,
                                 const void *land, const void *ice, void *out) {
    NEED(ctx, dtype == PGW_F32 || dtype == PGW_F64, "dtype must be PGW_F32 or PGW_F64");
    NEED(ctx, n >= 1 && tos && ts && land && ice && out, "bad argument");
    {
        Prof pr(ctx, PGW_K_SURFACE);
        with_type(dtype, [&](auto t_) {
            using T = decltype(t_);
            hipLaunchKernelGGL((k_integrate_tos<T>), dim3(nblocks(n, BLOCK)), dim3(BLOCK), 0, ctx->stream, n, (const T *)tos,
                               (const T *)ts, (const T *)land, (const T *)ice, (T *)out);
        });
    }
    HIPCHK(ctx, hipGetLastError());
    return PGW_OK;
}

extern "C" int pgw_surface_update(pgw_ctx *ctx, int dtype, int ntime, long long ncol, int nsoil,
                                  const double *soil_depth, const void *sic, const void *dsic, const void *dtos,
                                  const void *dts, const void *land, const void *ts_clim, const void *tskin,
                                  const void *tso, void *sic_out, void *dts_comb_out, void *tskin_out, void *tso_out) {
    CHECK_COMMON(ctx, dtype, ntime, ncol);
    SoilTable st;
    int rc;
    if ((rc = soil_table(ctx, __func__, nsoil, soil_depth, &st))) return rc;
    NEED(ctx, sic && dsic && dtos && dts && land, "null pointer");
    NEED(ctx, !tskin_out || tskin, "tskin required for tskin_out");
    NEED(ctx, !tso_out || (tso && ts_clim && soil_depth && nsoil > 0), "tso, ts_clim, soil_depth required for tso_out");
    long long n = (long long)ntime * ncol;
    {
        Prof pr(ctx, PGW_K_SURFACE);
        with_type(dtype, [&](auto t_) {
            using T = decltype(t_);
            // the deltas at the instant, already interpolated: records with nothing after them
            const RiderSrc<T> r{(const T *)sic, delta_src<T>(dsic, nullptr, 0.0, 0.0), delta_src<T>(dtos, nullptr, 0.0, 0.0),
                                delta_src<T>(dts, nullptr, 0.0, 0.0), (const T *)land};
            hipLaunchKernelGGL((k_surface_update_lerp<T, false>), dim3(nblocks(n, BLOCK)), dim3(BLOCK), 0, ctx->stream, ntime, ncol, st,
                               r, (const T *)ts_clim, (const T *)tskin, (const T *)tso, (T *)sic_out, (T *)dts_comb_out,
                               (T *)tskin_out, (T *)tso_out);
        });
    }
    HIPCHK(ctx, hipGetLastError());
    return PGW_OK;
}

// step_03 --debug_mode interpolate_full: delta_ts_combined (step_03:118-125) and delta_soilt (:139-143) as float64 arrays,
// every 2-D delta on its own time axis as in pgw_step03_file
extern "C" int pgw_surface_deltas(pgw_ctx *ctx, int dtype, int ref_dtype, int ntime, long long ncol, int nsoil,
                                  const double *soil_depth, const void *sic, const void *siconc_b, const void *siconc_a,
                                  double siconc_x_hi, double siconc_x_new, const void *tos_b, const void *tos_a,
                                  double tos_x_hi, double tos_x_new, const void *ts_b, const void *ts_a, double ts_x_hi,
                                  double ts_x_new, const void *land, const void *ts_clim, double *dts_comb,
                                  double *delta_soilt) {
    CHECK_COMMON(ctx, dtype, ntime, ncol);
    const bool ref = ref_dtype != 0;
    NEED(ctx, !ref || dtype == PGW_F32, "ref_dtype = 1 is the float32-file mode: dtype must be PGW_F32");
    SoilTable st;
    int rc;
    if ((rc = soil_table(ctx, __func__, nsoil, soil_depth, &st))) return rc;
    NEED(ctx, sic && siconc_b && tos_b && ts_b && land && dts_comb, "null pointer");
    NEED(ctx, (siconc_x_hi == 0.0 || siconc_a) && (tos_x_hi == 0.0 || tos_a) && (ts_x_hi == 0.0 || ts_a),
         "record after the instant is NULL");
    NEED(ctx, !delta_soilt || (ts_clim && soil_depth && nsoil > 0), "ts_clim, soil_depth required for delta_soilt");
    const long long n = (long long)ntime * ncol;
    {
        Prof pr(ctx, PGW_K_SURFACE);
        with_flow(dtype, ref, [&](auto t_, auto, auto ref_) {
            using T = decltype(t_);
            const RiderSrc<T> r{(const T *)sic, delta_src<T>(siconc_b, siconc_a, siconc_x_hi, siconc_x_new),
                                delta_src<T>(tos_b, tos_a, tos_x_hi, tos_x_new), delta_src<T>(ts_b, ts_a, ts_x_hi, ts_x_new),
                                (const T *)land};
            hipLaunchKernelGGL((k_surface_deltas<T, decltype(ref_)::value>), dim3(nblocks(n, BLOCK)), dim3(BLOCK), 0, ctx->stream,
                               ntime, ncol, st, r, (const T *)ts_clim, dts_comb, delta_soilt);
        });
    }
    HIPCHK(ctx, hipGetLastError());
    return PGW_OK;
}

// ================================================================== the reference's dtype flow, function level
// settings.function_dtype_flow = 'reference': one dtype tag per operand, nothing is cast up front; the kernels reproduce
// numpy's promotion through the cited reference lines (include/pgw_hip.h).  A tag combination that is not instantiated is
// PGW_ERR_ARG with a message, never another instantiation.

// Elements per thread of a kernel whose rows differ in element size: the narrowest row loads as one 16-byte (V = 4 float32)
// or 8-byte (V = 2) access per lane, a float64 row beside it as V / 2 16-byte accesses; all rows float64: V = 2 as in
// pick_vec.  PGW_OPT_MIXED_VEC caps V (A/B knob of tools/function_flow_time.py).
static int pick_vec_mixed(pgw_ctx *ctx, bool any_f32, long long ncol, std::initializer_list<const void *> ptrs) {
    int v = any_f32 ? 4 : 2;
    if (v > ctx->opt[PGW_OPT_MIXED_VEC]) v = ctx->opt[PGW_OPT_MIXED_VEC] < 1 ? 1 : ctx->opt[PGW_OPT_MIXED_VEC];
    if (v == 3) v = 2;
    return fit_vec(ctx, v, ncol, ptrs);
}

extern "C" int pgw_integ_geopot_mixed(pgw_ctx *ctx, int dt_pa_hl, int dt_zgs, int dt_ta, int dt_hus, int ntime, int nlev,
                                      long long ncol, const void *pa_hl, const void *zgs, const void *ta, const void *hus,
                                      double p_ref, const void *p_ref_field, double *phi_ref, int full_column) {
    NEED(ctx, TAG_OK(dt_pa_hl) && TAG_OK(dt_zgs) && TAG_OK(dt_ta) && TAG_OK(dt_hus), "dtype tags must be PGW_F32 or PGW_F64");
    NEED(ctx, dt_pa_hl == PGW_F64, "pgw_integ_geopot_mixed: float32 pa_hl / p_ref field (a float32 logarithm) is not instantiated");
    NEED(ctx, ntime >= 1 && ncol >= 1 && nlev >= 1, "ntime, nlev and ncol must be positive");
    NEED(ctx, pa_hl && zgs && ta && hus && phi_ref, "null pointer");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    int rc = status_reset(ctx);
    if (rc) return rc;
    const bool any32 = dt_ta == PGW_F32 || dt_hus == PGW_F32;
    const int vec = pick_vec_mixed(ctx, any32, ncol, {pa_hl, zgs, ta, hus, p_ref_field, phi_ref});
    {
        Prof pr(ctx, PGW_K_INTEG_GEOPOT);
        with_type(dt_zgs, [&](auto z_) { with_type(dt_ta, [&](auto t_) { with_type(dt_hus, [&](auto q_) { with_vec(vec, [&](auto v_) {
            using TZ = decltype(z_); using TT = decltype(t_); using TQ = decltype(q_);
            constexpr int V = decltype(v_)::value;
            if constexpr (V <= 2 || sizeof(TT) == 4 || sizeof(TQ) == 4)
                hipLaunchKernelGGL((k_integ_geopot<double, V, 4, double, TZ, TT, TQ, true>), dim3(nblocks((long long)ntime * ncol / V, BLOCK)),
                                   dim3(BLOCK), 0, ctx->stream, nlev, ntime, ncol, (const double *)pa_hl, (const TZ *)zgs,
                                   (const TT *)ta, (const TQ *)hus, p_ref, (const double *)p_ref_field, phi_ref, full_column,
                                   ctx->d_status);
        }); }); }); });
    }
    HIPCHK(ctx, hipGetLastError());
    return status_check(ctx);
}

template <int WHICH>
static void launch_humidity_mixed(pgw_ctx *ctx, int dt_a, int dt_b, int dt_c, long long n, const void *a, const void *b,
                                  const void *c, void *out) {
    const int vec = pick_vec_mixed(ctx, true, n, {a, b, c, out}) == 4 ? 4 : 1;
    const unsigned int nb = flat_grid(n / vec);
    with_type(dt_a, [&](auto a_) { with_type(dt_b, [&](auto b_) { with_type(dt_c, [&](auto c_) { with_vec(vec, [&](auto v_) {
        using TA = decltype(a_); using TB = decltype(b_); using TC = decltype(c_);
        constexpr int V = decltype(v_)::value;
        if constexpr (V != 2) {
            using TO = humidity_out_t<WHICH, TA, TB, TC>;
            hipLaunchKernelGGL((k_humidity_mixed<WHICH, TA, TB, TC, V>), dim3(nb), dim3(BLOCK), 0, ctx->stream, n, (const TA *)a,
                               (const TB *)b, (const TC *)c, (TO *)out);
        }
    }); }); }); });
}

extern "C" int pgw_humidity_mixed(pgw_ctx *ctx, int which, int dt_a, int dt_b, int dt_c, long long n, const void *a,
                                  const void *b, const void *c, void *out) {
    NEED(ctx, which >= 0 && which <= 6, "which must be 0..6");
    NEED(ctx, TAG_OK(dt_a) && TAG_OK(dt_b) && TAG_OK(dt_c), "dtype tags must be PGW_F32 or PGW_F64");
    NEED(ctx, n >= 1 && a && out && ((which >= 2 && which <= 4) || b) && (which < 5 || c), "bad argument");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    // operands a function does not take carry the tag of `a`: one instantiation per combination that exists
    if (which >= 2 && which <= 4) dt_b = dt_a;
    if (which < 5) dt_c = dt_a;
    {
        Prof pr(ctx, which == 6 ? PGW_K_RH_TO_Q : PGW_K_Q_TO_RH);
        with_int<7>(which, [&](auto w_) { launch_humidity_mixed<decltype(w_)::value>(ctx, dt_a, dt_b, dt_c, n, a, b, c, out); });
    }
    HIPCHK(ctx, hipGetLastError());
    return PGW_OK;
}

extern "C" int pgw_interp_logp_4d_mixed(pgw_ctx *ctx, int dt_var, int dt_p, int ntime, int nsrc, int ntarg, long long ncol,
                                        const void *var, const void *source_P, const void *targ_P, int extrapolate,
                                        int logp_in, double *out) {
    NEED(ctx, TAG_OK(dt_var) && TAG_OK(dt_p), "dtype tags must be PGW_F32 or PGW_F64");
    NEED(ctx, dt_p == PGW_F64, "pgw_interp_logp_4d_mixed: float32 pressures (a float32 logarithm) are not instantiated");
    NEED(ctx, ntime >= 1 && ncol >= 1, "ntime and ncol must be positive");
    NEED(ctx, nsrc >= 2 && ntarg >= 1, "need at least 2 source levels and 1 target level");
    NEED(ctx, var && source_P && targ_P && out, "null pointer");
    if (extrapolate < 0 || extrapolate > 3) return fail(ctx, PGW_ERR_ARG, "Invalid input value for \"extrapolate\"");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    int rc = status_reset(ctx);
    if (rc) return rc;
    const long long total = (long long)ntime * ncol;
    {
        Prof pr(ctx, PGW_K_INTERP_LOGP);
        with_type(dt_var, [&](auto v_) { with_int<4>(extrapolate, [&](auto m_) {
            using TV = decltype(v_);
            hipLaunchKernelGGL((k_interp_logp_stream<TV, double, double, decltype(m_)::value>), dim3(nblocks(total, BLOCK)), dim3(BLOCK),
                               0, ctx->stream, ntime, nsrc, ntarg, ncol, (const TV *)var, (const double *)source_P,
                               (const double *)targ_P, out, logp_in, ctx->d_status);
        }); });
    }
    HIPCHK(ctx, hipGetLastError());
    return status_check(ctx);
}

extern "C" int pgw_vert_interp_delta_mixed(pgw_ctx *ctx, int dt_delta, int dt_sfc, int dt_pshist, int dt_targ, int dt_add,
                                           int ntime, int nplev, int nlev_t, long long ncol, const double *plev,
                                           const void *delta, const void *delta_sfc, const void *ps_hist, const void *targ_P,
                                           int ignore_top, const void *add_to, double *out) {
    NEED(ctx, TAG_OK(dt_delta) && TAG_OK(dt_sfc) && TAG_OK(dt_pshist) && TAG_OK(dt_targ) && TAG_OK(dt_add),
         "dtype tags must be PGW_F32 or PGW_F64");
    NEED(ctx, dt_targ == PGW_F64, "pgw_vert_interp_delta_mixed: float32 target pressures (a float32 logarithm) are not instantiated");
    NEED(ctx, ntime >= 1 && ncol >= 1 && nlev_t >= 1, "ntime, nlev_t and ncol must be positive");
    NEED(ctx, nplev >= 2 && nplev <= MAX_PLEV_WIDE, PLEV_RANGE_2);
    NEED(ctx, plev && delta && targ_P && out, "null pointer");
    NEED(ctx, (delta_sfc == nullptr) == (ps_hist == nullptr), "delta_sfc and ps_hist must be given together");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    int rc = plev_table(ctx, nplev, plev);
    if (rc) return rc;
    rc = status_reset(ctx);
    if (rc) return rc;
    Levels lv = levels_of(ctx);
    lv.akm = lv.bkm = nullptr;
    const long long total = (long long)ntime * ncol;
    if (!add_to) dt_add = PGW_F64;
    if (!delta_sfc) { dt_sfc = dt_delta; dt_pshist = PGW_F64; }
    {
        Prof pr(ctx, PGW_K_VERT_INTERP_DELTA);
        with_type(dt_delta, [&](auto d_) { with_type(dt_add, [&](auto a_) { with_plev(ctx, [&](const auto &pt) {
            using TD = decltype(d_); using TA = decltype(a_); using PT = std::decay_t<decltype(pt)>;
            const DeltaSrc<TD> d = delta_src<TD>(delta, nullptr, 0.0, 0.0);           // the records of the instant itself
            if (!delta_sfc) {
                const DeltaSrc<TD> s = delta_src<TD>(nullptr, nullptr, 0.0, 0.0);
                const DeltaSrc<double> p = delta_src<double>(nullptr, nullptr, 0.0, 0.0);
                hipLaunchKernelGGL((k_vert_interp_delta<TD, double, double, false, TA, TD, double, PT>), dim3(nblocks(total, BLOCK)), dim3(BLOCK),
                                   0, ctx->stream, pt, lv, ntime, nlev_t, ncol, d, s, p, (const double *)targ_P,
                                   (const double *)nullptr, ignore_top ? 0 : 1, (const TA *)add_to, out, ctx->d_status);
            } else {
                with_type(dt_sfc, [&](auto s_) { with_type(dt_pshist, [&](auto h_) {
                    using TS = decltype(s_); using TH = decltype(h_);
                    const DeltaSrc<TS> s = delta_src<TS>(delta_sfc, nullptr, 0.0, 0.0);
                    const DeltaSrc<TH> p = delta_src<TH>(ps_hist, nullptr, 0.0, 0.0);
                    hipLaunchKernelGGL((k_vert_interp_delta<TD, double, double, true, TA, TS, TH, PT>), dim3(nblocks(total, BLOCK)), dim3(BLOCK),
                                       0, ctx->stream, pt, lv, ntime, nlev_t, ncol, d, s, p, (const double *)targ_P,
                                       (const double *)nullptr, ignore_top ? 0 : 1, (const TA *)add_to, out, ctx->d_status);
                }); });
            }
        }); }); });
    }
    HIPCHK(ctx, hipGetLastError());
    rc = status_check(ctx);
    if (rc) return rc;
    return top_pressure_check(ctx, ignore_top);
}

extern "C" int pgw_replace_delta_sfc_mixed(pgw_ctx *ctx, int dt_delta, int dt_sfc, int dt_pshist, int ntime, int nplev,
                                           long long ncol, const double *plev_asc, const void *delta, const void *delta_sfc,
                                           const void *ps_hist, double *out_P, void *out_delta) {
    NEED(ctx, TAG_OK(dt_delta) && TAG_OK(dt_sfc) && TAG_OK(dt_pshist), "dtype tags must be PGW_F32 or PGW_F64");
    NEED(ctx, ntime >= 1 && ncol >= 1, "ntime and ncol must be positive");
    NEED(ctx, nplev >= 1 && nplev <= MAX_PLEV_WIDE, PLEV_RANGE_1);
    NEED(ctx, plev_asc && delta && delta_sfc && ps_hist && out_P && out_delta, "null pointer");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const PlevTableWide tw = ascending_plev_table(nplev, plev_asc);
    int rc = status_reset(ctx);
    if (rc) return rc;
    const long long total = (long long)ntime * ncol;
    {
        Prof pr(ctx, PGW_K_VERT_INTERP_DELTA);
        with_type(dt_delta, [&](auto d_) { with_type(dt_sfc, [&](auto s_) { with_type(dt_pshist, [&](auto h_) { with_plev(tw, [&](const auto &pt) {
            using TD = decltype(d_); using TS = decltype(s_); using TH = decltype(h_);
            hipLaunchKernelGGL((k_replace_delta_sfc<TD, TS, TH, double, std::decay_t<decltype(pt)>>), dim3(nblocks(total, BLOCK)), dim3(BLOCK), 0, ctx->stream, pt,
                               ntime, ncol, (const TD *)delta, (const TS *)delta_sfc, (const TH *)ps_hist, out_P, (TD *)out_delta,
                               ctx->d_status);
        }); }); }); });
    }
    HIPCHK(ctx, hipGetLastError());
    return status_check(ctx);
}

extern "C" int pgw_time_lerp_mixed(pgw_ctx *ctx, int dt_before, int dt_after, long long n, const void *v_before,
                                   const void *v_after, double x_hi, double x_new, double *out) {
    NEED(ctx, TAG_OK(dt_before) && TAG_OK(dt_after), "dtype tags must be PGW_F32 or PGW_F64");
    NEED(ctx, n >= 1 && v_before && v_after && out, "bad argument");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const int vec = pick_vec_mixed(ctx, dt_before == PGW_F32 || dt_after == PGW_F32, n, {v_before, v_after, out}) >= 2 ? 2 : 1;
    const unsigned int nb = flat_grid(n / vec);
    {
        Prof pr(ctx, PGW_K_TIME_LERP);
        with_type(dt_before, [&](auto b_) { with_type(dt_after, [&](auto a_) { with_vec(vec, [&](auto v_) {
            using TB = decltype(b_); using TA = decltype(a_);
            constexpr int V = decltype(v_)::value;
            if constexpr (V <= 2)
                hipLaunchKernelGGL((k_time_lerp<TB, V, TA, double, true>), dim3(nb), dim3(BLOCK), 0, ctx->stream, n, (const TB *)v_before,
                                   (const TA *)v_after, x_hi, x_new, out);
        }); }); });
    }
    HIPCHK(ctx, hipGetLastError());
    return PGW_OK;
}

extern "C" int pgw_integrate_tos_mixed(pgw_ctx *ctx, int dt_tos, int dt_ts, int dt_land, int dt_ice, long long n,
                                       const void *tos, const void *ts, const void *land, const void *ice, double *out) {
    NEED(ctx, TAG_OK(dt_tos) && TAG_OK(dt_ts) && TAG_OK(dt_land) && TAG_OK(dt_ice), "dtype tags must be PGW_F32 or PGW_F64");
    NEED(ctx, n >= 1 && tos && ts && land && ice && out, "bad argument");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    {
        Prof pr(ctx, PGW_K_SURFACE);
        with_type(dt_tos, [&](auto o_) { with_type(dt_ts, [&](auto s_) { with_type(dt_land, [&](auto l_) { with_type(dt_ice, [&](auto i_) {
            using TO_ = decltype(o_); using TS = decltype(s_); using TL = decltype(l_); using TI = decltype(i_);
            hipLaunchKernelGGL((k_integrate_tos_mixed<TO_, TS, TL, TI>), dim3(nblocks(n, BLOCK)), dim3(BLOCK), 0, ctx->stream, n,
                               (const TO_ *)tos, (const TS *)ts, (const TL *)land, (const TI *)ice, out);
        }); }); }); });
    }
    HIPCHK(ctx, hipGetLastError());
    return PGW_OK;
}
