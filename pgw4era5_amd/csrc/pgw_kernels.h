// pgw_kernels.h -- hand-written gfx950 kernels for the PGW4ERA5 step_03 / step_02 hot path.
// All arithmetic is IEEE fp64 (no fast-math); T is the storage type of field arrays.
// Citations are reference file:line (functions.py unless prefixed).
#pragma once
#include "pgw_device.h"

namespace pgw {

// Signature-faithful streaming kernels read and write each element once: streaming (non-temporal) forms (pgw_device.h)
#define SIG_LOADV loadv_nt
#define SIG_LD(p) __builtin_nontemporal_load(p)
#define SIG_ST(v, p) __builtin_nontemporal_store((v), (p))

// Vertical-grid tables of a context, in device memory; every access is wave-uniform
// (index = level loop counter) so the compiler emits scalar (s_load) reads.
struct Levels {
    const double *ak;    // nlev+1
    const double *bk;    // nlev+1
    const double *akm;   // nlev
    const double *bkm;   // nlev
    int nlev;
    double ps_mono_min;  // columns with ps >= this have strictly ascending half-level pressure
};

// The tables are staged in LDS by every kernel that walks levels: a coefficient read through the
// kernel-argument pointer compiles to a VECTOR global load (the compiler cannot prove the table is
// not aliased by the kernel's stores), and its `s_waitcnt vmcnt` then also waits for every
// prefetched row and earlier store of the wave (vmcnt retires in order) - one such load per level
// serialises the whole software pipeline.  ds_read uses lgkmcnt and leaves vmcnt traffic in flight.
constexpr int MAX_NLEV = 256;
struct LevTab {            // LDS image: ak[0..N] | bk[0..N] | akm[0..N-1] | bkm[0..N-1] | table of pgw_log_tab
    const double *ak, *bk, *akm, *bkm, *logtab;
};
template <bool HALF, bool FULL>
__device__ __forceinline__ LevTab stage_levels(const Levels &lv, double *lds, int nthreads) {
    const int N = lv.nlev;
    LevTab t;
    t.ak = lds; t.bk = lds + (MAX_NLEV + 1); t.akm = lds + 2 * (MAX_NLEV + 1); t.bkm = t.akm + MAX_NLEV;
    t.logtab = t.bkm + MAX_NLEV;
    stage_log_table(lds + 2 * (MAX_NLEV + 1) + 2 * MAX_NLEV, nthreads);
    double *w = lds;
    for (int i = threadIdx.x; i <= N; i += nthreads) {
        if (HALF) { w[i] = lv.ak[i]; w[(MAX_NLEV + 1) + i] = lv.bk[i]; }
        if (FULL && i < N) { w[2 * (MAX_NLEV + 1) + i] = lv.akm[i]; w[2 * (MAX_NLEV + 1) + MAX_NLEV + i] = lv.bkm[i]; }
    }
    __syncthreads();
    return t;
}
constexpr int LEVTAB_DOUBLES = 2 * (MAX_NLEV + 1) + 2 * MAX_NLEV + 2 * LOG_TABLE_N;

// flat column group -> (time, column) and base offsets
struct ColIdx {
    long long t, c;
};
__device__ __forceinline__ ColIdx col_index(long long g, int V, long long ncol) {
    long long flat = g * V;
    ColIdx r;
    r.t = flat / ncol;
    r.c = flat - r.t * ncol;
    return r;
}

// =====================================================================================
// a1  pressure on half / full levels          step_03_apply_to_era.py:64-66,87-88,196-199
// write-bound: (2N+1) rows out per column, 1 element in.
// =====================================================================================
template <typename T, int V>
__global__ __launch_bounds__(BLOCK) void k_pressure_levels(Levels lv, int ntime, long long ncol,
                                                           const T *__restrict__ ps,
                                                           T *__restrict__ pa_hl, T *__restrict__ pa) {
    __shared__ double s_lev[LEVTAB_DOUBLES];
    LevTab lt = stage_levels<true, true>(lv, s_lev, BLOCK);
    long long g = (long long)blockIdx.x * BLOCK + threadIdx.x;
    long long ngroups = (long long)ntime * ncol / V;
    if (g >= ngroups) return;
    ColIdx ix = col_index(g, V, ncol);
    double p[V];
    loadv<T, V>(ps + ix.t * ncol + ix.c, p);
    const int N = lv.nlev;
    if (pa_hl) {
        T *o = pa_hl + ix.t * (N + 1) * ncol + ix.c;
#pragma unroll 4
        for (int k = 0; k <= N; ++k) {
            double a = lt.ak[k], b = lt.bk[k], r[V];
#pragma unroll
            for (int v = 0; v < V; ++v) r[v] = a + p[v] * b;
            storev<T, V>(o + (long long)k * ncol, r);
        }
    }
    if (pa) {
        T *o = pa + ix.t * N * ncol + ix.c;
#pragma unroll 4
        for (int l = 0; l < N; ++l) {
            double a = lt.akm[l], b = lt.bkm[l], r[V];
#pragma unroll
            for (int v = 0; v < V; ++v) r[v] = a + p[v] * b;
            storev<T, V>(o + (long long)l * ncol, r);
        }
    }
}

// =====================================================================================
// a2 / a3  humidity conversions, flat elementwise             functions.py:107-125
// MODE 0: q -> RH ; MODE 1: RH -> q ; MODE 2: RH -> e (vapour pressure, :123)
// =====================================================================================
template <typename T, int V, int MODE>
__global__ __launch_bounds__(BLOCK) void k_humidity_flat(long long n, const T *__restrict__ x,
                                                         const T *__restrict__ pa,
                                                         const T *__restrict__ ta, T *__restrict__ out) {
    long long stride = (long long)gridDim.x * BLOCK;
    for (long long g = (long long)blockIdx.x * BLOCK + threadIdx.x; g * V < n; g += stride) {
        double a[V], p[V], t[V], r[V];
        loadv<T, V>(x + g * V, a);
        loadv<T, V>(pa + g * V, p);
        loadv<T, V>(ta + g * V, t);
#pragma unroll
        for (int v = 0; v < V; ++v) r[v] = (MODE == 0) ? q_to_rh(a[v], p[v], t[v]) : rh_to_q(a[v], p[v], t[v]);
        storev<T, V>(out + g * V, r);
    }
}

// the leaf helpers (functions.py:58-105), literal forms with IEEE divisions
template <typename T, int WHICH>
__global__ __launch_bounds__(BLOCK) void k_humidity_leaf(long long n, const T *__restrict__ a, const T *__restrict__ b,
                                                         T *__restrict__ out) {
    long long stride = (long long)gridDim.x * BLOCK;
    for (long long i = (long long)blockIdx.x * BLOCK + threadIdx.x; i < n; i += stride) {
        const double x = (double)a[i];
        double r;
        if (WHICH == 0) { const double p = (double)b[i]; r = x * p / (CON_MW_MD + 0.378 * x); }
        else if (WHICH == 1) { const double p = (double)b[i]; r = CON_MW_MD * x / (p - (1 - CON_MW_MD) * x); }
        else if (WHICH == 2) r = 611.21 * pgw_exp(17.502 * (x - 273.16) / (x - 32.19));
        else if (WHICH == 3) r = 611.21 * pgw_exp(22.587 * (x - 273.16) / (x - (-0.7)));
        else r = esat_mixed(x);
        out[i] = (T)r;
    }
}

// The humidity functions in the reference's dtype flow (settings.function_dtype_flow = 'reference'): every operand in its
// own storage type, the expression in numpy's promoted type at every node (humidity_expr, pgw_device.h), the result in
// the promoted type of the whole expression.  b / c are not read by the functions that do not take them.
template <int WHICH, typename TA, typename TB, typename TC, int V>
__global__ __launch_bounds__(BLOCK) void k_humidity_mixed(long long n, const TA *__restrict__ a, const TB *__restrict__ b,
                                                          const TC *__restrict__ c,
                                                          humidity_out_t<WHICH, TA, TB, TC> *__restrict__ out) {
    using TO = humidity_out_t<WHICH, TA, TB, TC>;
    static_assert(std::is_same<TO, decltype(humidity_expr<WHICH>(TA(), TB(), TC()))>::value, "humidity_out_t");
    long long stride = (long long)gridDim.x * BLOCK;
    for (long long g = (long long)blockIdx.x * BLOCK + threadIdx.x; g * V < n; g += stride) {
        TA x[V]; TB y[V]; TC z[V]; TO r[V];
        loadv_typed<TA, V>(a + g * V, x);
        if constexpr (WHICH <= 1 || WHICH >= 5) loadv_typed<TB, V>(b + g * V, y);
        if constexpr (WHICH >= 5) loadv_typed<TC, V>(c + g * V, z);
#pragma unroll
        for (int v = 0; v < V; ++v) {
            if constexpr (WHICH >= 5) r[v] = humidity_expr<WHICH>(x[v], y[v], z[v]);
            else if constexpr (WHICH <= 1) r[v] = humidity_expr<WHICH>(x[v], y[v], TC());
            else r[v] = humidity_expr<WHICH>(x[v], TB(), TC());
        }
        storev_typed<TO, V>(out + g * V, r);
    }
}

// RELHUM of a float32 ERA state in reference-dtype mode (step_03:91-94 on a float32 file): float32 QV, T, PS in, the float64
// field numpy's promotion produces out (q_to_rh_f32: float64 pressure, float32 e_sat chain)
__global__ __launch_bounds__(BLOCK) void k_relhum_ref(Levels lv, int ntime, long long ncol, const float *__restrict__ hus,
                                                      const float *__restrict__ ps, const float *__restrict__ ta,
                                                      double *__restrict__ out) {
    __shared__ double s_lev[LEVTAB_DOUBLES];
    LevTab lt = stage_levels<false, true>(lv, s_lev, BLOCK);
    long long g = (long long)blockIdx.x * BLOCK + threadIdx.x;
    if (g >= (long long)ntime * ncol) return;
    const long long t = g / ncol, c = g - t * ncol;
    const double p = (double)ps[g];
    const int N = lv.nlev;
    const long long base = t * N * ncol + c;
#pragma unroll 4
    for (int l = 0; l < N; ++l) {
        const long long o = base + (long long)l * ncol;
        out[o] = q_to_rh_f32(hus[o], lt.akm[l] + p * lt.bkm[l], ta[o]);
    }
}

// same with pa = akm + ps*bkm rebuilt in registers (no 4-D pressure array)
template <typename T, int V, int MODE>
__global__ __launch_bounds__(BLOCK) void k_humidity_hybrid(Levels lv, int ntime, long long ncol,
                                                           const T *__restrict__ x, const T *__restrict__ ps,
                                                           const T *__restrict__ ta, T *__restrict__ out) {
    __shared__ double s_lev[LEVTAB_DOUBLES];
    LevTab lt = stage_levels<false, true>(lv, s_lev, BLOCK);
    long long g = (long long)blockIdx.x * BLOCK + threadIdx.x;
    long long ngroups = (long long)ntime * ncol / V;
    if (g >= ngroups) return;
    ColIdx ix = col_index(g, V, ncol);
    double p[V];
    loadv<T, V>(ps + ix.t * ncol + ix.c, p);
    const int N = lv.nlev;
    long long base = ix.t * N * ncol + ix.c;
#pragma unroll 2
    for (int l = 0; l < N; ++l) {
        double a[V], t[V], r[V];
        loadv<T, V>(x + base + (long long)l * ncol, a);
        loadv<T, V>(ta + base + (long long)l * ncol, t);
        double am = lt.akm[l], bm = lt.bkm[l];
#pragma unroll
        for (int v = 0; v < V; ++v) {
            double pa = am + p[v] * bm;
            r[v] = (MODE == 0) ? q_to_rh(a[v], pa, t[v]) : (MODE == 1) ? rh_to_q(a[v], pa, t[v]) : rh_to_e(a[v], t[v]);
        }
        storev<T, V>(out + base + (long long)l * ncol, r);
    }
}

// =====================================================================================
// a4  integ_geopot                                             functions.py:128-189
// One thread = V columns, bottom-up scan; the half level k* with the smallest non-negative
// p_hl - p_ref (ties -> lowest k, like nanargmin) is tracked while scanning, so non-monotone
// columns give the reference's answer too.
// =====================================================================================
struct GeoAcc {            // per-column running state of the upward scan
    double phi;            // phi at the lower half level of the current layer
    double p_lo, lnp_lo;   // pressure / ln p at that half level
    double dmin;           // smallest non-negative p_hl - p_ref so far
    double phi_s, rtv_s, lnp_s;   // phi, CON_RD*tv and ln p captured at the candidate k*
    double p_s;            // the pressure itself there (geo_layer<.., .., CAP = true> only, for geo_finish_exact)
    int kstar;             // -1 = none yet
};

// Reference-dtype mode (REF, float32 ERA5 files): `phi_hl` is created from the float32
// `zgs` (functions.py:141), so every assignment phi_hl[l] = ... (:149-152) rounds to float32; `tav` and `CON_RD * tav`
// are float32 products for the float32 ERA state (:144, :150).  All of these are single IEEE operations, reproduced
// exactly: cvt f64->f32->f64 for the store, v_mul_f32 / v_add_f32 for the products (-ffp-contract=off).
template <bool REF>
__device__ __forceinline__ double phi_store(double x) { return REF ? (double)(float)x : x; }
// CON_RD * (ta * (1 + 0.61 * hus)) for float32 ta, hus as numpy evaluates it: python floats become float32 scalars
__device__ __forceinline__ double rd_tv_f32(double t, double q) {
    const float tv = (float)t * (1.0f + 0.61f * (float)q);       // :144
    return (double)(287.05f * tv);                               // :150  CON_RD * tav.sel(...)
}

// `logtab`: LDS table of pgw_log_tab (the hybrid-level kernels), or nullptr: fdlibm kernel (pgw_log)
__device__ __forceinline__ void geo_init(GeoAcc &a, double zgs, double p_bottom, const double *logtab = nullptr) {
    a.phi = zgs;
    a.p_lo = fix_p(p_bottom);
    a.lnp_lo = logtab ? pgw_log_tab(a.p_lo, logtab) : pgw_log(a.p_lo);
    a.dmin = __builtin_inf();
    a.kstar = -1;
    a.phi_s = a.rtv_s = a.lnp_s = 0.0;
    a.p_s = 1.0;
}
// process layer l (between half levels l and l+1); rtv = CON_RD * tv of the layer; p_top = pa_hl[l] raw
template <bool REF = false, bool TAB = false, bool CAP = false>
__device__ __forceinline__ void geo_layer(GeoAcc &a, int l, double rtv, double p_top, double p_ref, const double *logtab = nullptr) {
    double d = a.p_lo - p_ref;                        // candidate k = l+1         :160-161
    if (d >= 0 && d <= a.dmin) {
        a.dmin = d; a.kstar = l + 1; a.phi_s = a.phi; a.rtv_s = rtv; a.lnp_s = a.lnp_lo;
        if (CAP) a.p_s = a.p_lo;
    }
    double p_hi = fix_p(p_top);                       // :135
    double lnp_hi = TAB ? pgw_log_tab(p_hi, logtab) : pgw_log_f3(p_hi);      // the log of the level loops
    a.phi = phi_store<REF>(a.phi + rtv * (a.lnp_lo - lnp_hi));   // :149-152, dlnpa :136-138
    a.p_lo = p_hi; a.lnp_lo = lnp_hi;
}
// returns phi_ref; reports errors
__device__ __forceinline__ double geo_finish(GeoAcc &a, double p_ref, DevStatus *st, long long col) {
    double d = a.p_lo - p_ref;                        // candidate k = 0
    if (d >= 0 && d <= a.dmin) a.kstar = 0;
    if (a.kstar < 0) { report(st, 13 /*PGW_ERR_PREF_BELOW_SURFACE*/, col); return __builtin_nan(""); }
    if (a.kstar == 0) { report(st, 14 /*PGW_ERR_PREF_AT_TOP*/, col); return __builtin_nan(""); }
    return a.phi_s - a.rtv_s * (pgw_log(p_ref) - a.lnp_s);    // :174-179
}

// geo_finish for the reference's dtype flow of the function-level API: the final expression (:174-179) is float64 and no
// float32 rounding follows it, so the last bit of its two logarithms is the last bit of the result - they are taken with
// pgw_log_dd (numpy's bits for all but a few in 10^4 arguments) from the pressures themselves (CAP)
__device__ __forceinline__ double geo_finish_exact(GeoAcc &a, double p_ref, DevStatus *st, long long col) {
    double d = a.p_lo - p_ref;
    if (d >= 0 && d <= a.dmin) a.kstar = 0;
    if (a.kstar < 0) { report(st, 13 /*PGW_ERR_PREF_BELOW_SURFACE*/, col); return __builtin_nan(""); }
    if (a.kstar == 0) { report(st, 14 /*PGW_ERR_PREF_AT_TOP*/, col); return __builtin_nan(""); }
    return a.phi_s - a.rtv_s * (pgw_log_dd(p_ref) - pgw_log_dd(a.p_s));
}

// The same scan for columns whose half-level pressures are known to ascend (ps >= Levels::ps_mono_min), in fewer live
// registers (k_delta_quad carries it beside its own state), for NS states that share their half-level pressures (the ERA
// state and the PGW state of the loop's first pass, where delta_ps = 0): one fix_p, one logarithm and one k* test per
// level serve all of them.  In such a column d = p_lo - p_ref only falls on the way up, so every half level with d >= 0
// replaces the candidate before it (`d <= dmin` always holds) and k* is the last of them: instead of capturing
// (phi_s, rtv_s, lnp_s) the candidate's phi_ref is formed at once, with geo_finish's expression on the operands
// geo_layer would have captured, and dmin is not needed.  Same operations on the same values: same bits.
template <int NS>
struct GeoMono {
    double phi[NS];        // phi at the lower half level of the current layer
    double cand[NS];       // phi_ref if the current candidate is k*
    double p_lo, lnp_lo;   // pressure / ln p at that half level
    bool have;             // a candidate exists (geo_layer's kstar >= 0)
};
template <int NS>
__device__ __forceinline__ void geo_mono_init(GeoMono<NS> &a, double zgs, double p_bottom, const double *logtab) {
#pragma unroll
    for (int i = 0; i < NS; ++i) { a.phi[i] = zgs; a.cand[i] = 0.0; }
    a.p_lo = fix_p(p_bottom);
    a.lnp_lo = pgw_log_tab(a.p_lo, logtab);
    a.have = false;
}
// lnp_ref = pgw_log(p_ref), geo_finish's logarithm
template <bool REF, int NS>
__device__ __forceinline__ void geo_mono_layer(GeoMono<NS> &a, const double (&rtv)[NS], double p_top, double p_ref, double lnp_ref,
                                               const double *logtab) {
    double d = a.p_lo - p_ref;
    if (d >= 0) {
        a.have = true;
#pragma unroll
        for (int i = 0; i < NS; ++i) a.cand[i] = a.phi[i] - rtv[i] * (lnp_ref - a.lnp_lo);
    }
    double p_hi = fix_p(p_top);
    double lnp_hi = pgw_log_tab(p_hi, logtab);
#pragma unroll
    for (int i = 0; i < NS; ++i) a.phi[i] = phi_store<REF>(a.phi[i] + rtv[i] * (a.lnp_lo - lnp_hi));
    a.p_lo = p_hi; a.lnp_lo = lnp_hi;
}
template <int NS>
__device__ __forceinline__ double geo_mono_finish(const GeoMono<NS> &a, int i, double p_ref, DevStatus *st, long long col) {
    double d = a.p_lo - p_ref;                        // candidate k = 0: the model top is not above p_ref
    if (d >= 0) { report(st, 14 /*PGW_ERR_PREF_AT_TOP*/, col); return __builtin_nan(""); }
    if (!a.have) { report(st, 13 /*PGW_ERR_PREF_BELOW_SURFACE*/, col); return __builtin_nan(""); }
    return a.cand[i];
}

// Numpy's promotion of `CON_RD * (ta * (1 + 0.61 * hus))` (functions.py:144, :150) for storage types TT / TQ: a python float
// takes the dtype of the array it meets, so 1 + 0.61*hus is evaluated in TQ, the product with ta in the promoted type of
// (TT, TQ) - C++'s usual arithmetic conversions on float / double operands - and CON_RD in that type.  Both float: rd_tv_f32.
template <typename TT, typename TQ>
__device__ __forceinline__ double rd_tv_promoted(double t, double q) {
    if constexpr (sizeof(TT) == 4 && sizeof(TQ) == 4) return rd_tv_f32(t, q);
    else if constexpr (sizeof(TQ) == 4) return CON_RD * (t * (double)(1.0f + 0.61f * (float)q));     // float64 ta, float32 hus
    else return CON_RD * (t * (1 + 0.61 * q));
}

// Per-operand storage types: TP half-level pressures and a p_ref field, TZ zgs, TT / TQ the state, TO the phi_ref output
// (TP for the signature-faithful call, double for the loop state).  REF = false: float64 arithmetic on the stored values
// whatever the types (settings.function_dtype_flow = 'common': one type for all operands).  REF = true: the reference's
// dtype flow - phi_hl rounded to TZ at every level (phi_store), CON_RD * tav in the promoted type of (TT, TQ), logarithms
// and the final expression float64.  A thread owns V columns: a row of 8-byte elements is then V / 2 16-byte accesses.
template <typename TP, int V, int U, typename TO, typename TZ = TP, typename TT = TP, typename TQ = TT, bool REF = false>
__global__ __launch_bounds__(BLOCK) void k_integ_geopot(int nlev, int ntime, long long ncol,
                                                        const TP *__restrict__ pa_hl, const TZ *__restrict__ zgs,
                                                        const TT *__restrict__ ta, const TQ *__restrict__ hus,
                                                        double p_ref_s, const TP *__restrict__ p_ref_f,
                                                        TO *__restrict__ phi_ref, int full_column,
                                                        DevStatus *st) {
    constexpr bool PHI32 = REF && sizeof(TZ) == 4;
    long long g = (long long)blockIdx.x * BLOCK + threadIdx.x;
    long long ngroups = (long long)ntime * ncol / V;
    if (g >= ngroups) return;
    ColIdx ix = col_index(g, V, ncol);
    const int N = nlev;
    const TP *ph = pa_hl + ix.t * (N + 1) * ncol + ix.c;
    const TT *pt = ta + ix.t * N * ncol + ix.c;
    const TQ *pq = hus + ix.t * N * ncol + ix.c;
    long long c2 = ix.t * ncol + ix.c;
    double z[V], pb[V], pref[V];
    loadv16<TZ, V>(zgs + c2, z);
    loadv16<TP, V>(ph + (long long)N * ncol, pb);
    if (p_ref_f) loadv16<TP, V>(p_ref_f + c2, pref);
    else {
#pragma unroll
        for (int v = 0; v < V; ++v) pref[v] = p_ref_s;
    }
    GeoAcc acc[V];
#pragma unroll
    for (int v = 0; v < V; ++v) geo_init(acc[v], z[v], pb[v]);
    int l = N - 1;
    // chunks of U levels: issue all 3*U row loads, then the dependent scan
    for (; l >= U - 1; l -= U) {
        double p[U][V], t[U][V], q[U][V];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            SIG_LOADV<TP, V>(ph + (long long)(l - u) * ncol, p[u]);
            SIG_LOADV<TT, V>(pt + (long long)(l - u) * ncol, t[u]);
            SIG_LOADV<TQ, V>(pq + (long long)(l - u) * ncol, q[u]);
        }
        bool above = true;
#pragma unroll
        for (int u = 0; u < U; ++u) {
#pragma unroll
            for (int v = 0; v < V; ++v) {
                double rtv;
                if constexpr (REF) rtv = rd_tv_promoted<TT, TQ>(t[u][v], q[u][v]);
                else rtv = CON_RD * (t[u][v] * (1 + 0.61 * q[u][v]));          // :144
                geo_layer<PHI32, false, REF>(acc[v], l - u, rtv, p[u][v], pref[v]);
            }
        }
        if (!full_column) {
            // a column is finished once its pressure has dropped below p_ref and it has been
            // strictly ascending so far (then no higher half level can satisfy p >= p_ref)
#pragma unroll
            for (int v = 0; v < V; ++v) above = above && (acc[v].p_lo < pref[v]) && (acc[v].kstar >= 0);
            if (__all(above)) { l -= U; goto done; }
        }
    }
    for (; l >= 0; --l) {
        double p[V], t[V], q[V];
        SIG_LOADV<TP, V>(ph + (long long)l * ncol, p);
        SIG_LOADV<TT, V>(pt + (long long)l * ncol, t);
        SIG_LOADV<TQ, V>(pq + (long long)l * ncol, q);
#pragma unroll
        for (int v = 0; v < V; ++v) {
            double rtv;
            if constexpr (REF) rtv = rd_tv_promoted<TT, TQ>(t[v], q[v]);
            else rtv = CON_RD * (t[v] * (1 + 0.61 * q[v]));
            geo_layer<PHI32, false, REF>(acc[v], l, rtv, p[v], pref[v]);
        }
    }
done:
    double r[V];
#pragma unroll
    for (int v = 0; v < V; ++v) r[v] = REF ? geo_finish_exact(acc[v], pref[v], st, c2 + v) : geo_finish(acc[v], pref[v], st, c2 + v);
    storev16<TO, V>(phi_ref + c2, r);
}

// =====================================================================================
// a5  fused pass of the surface-pressure loop         step_03_apply_to_era.py:192-308
// The vapour pressure e = hur_pgw/100 * e_sat(ta_pgw) (functions.py:123) does not depend on
// the iterate, so it is precomputed once per file (k_humidity_hybrid MODE 2) and each pass
// does q = 0.622 e / (pa - 0.378 e) (:66-72) - the same values the reference recomputes.
// State (delta_ps, adj_ps) and the constant phi_ref_era / dphi_clim are fp64.
// =====================================================================================
// Upward scan of V hybrid-pressure columns from the surface to p_ref: shared by the loop pass
// (second field = vapour pressure e, q = e_to_q(e, pa)) and by phi_ref of the ERA state (second
// field = QV itself).  Levels are processed in chunks of U with the next chunk's 2*U row loads
// already in flight (software pipeline; ~2*U KiB per wave outstanding).
// TL = storage type of the two level arrays.  REF (reference-dtype mode, float32 files): phi rounded to float32 per
// level; for the ERA state (SECOND_IS_Q, float32 T and QV) tav and CON_RD*tav are float32 products.
// QMODE 2 = STORE_Q (loop pass only): the pass also stores the q it forms, as TL, for every level lc >= l_lim it processes (l_lim =
// nlev: none), lanes with `live` only, into the array of pe's shape that lies `qdiff` bytes behind it (hus_pgw: one uniform
// register pair instead of a second per-lane address); `low` returns the lowest level index the wave processed (the stop
// is wave-uniform: the same for all 64 lanes).  See k_ps_loop_multi.
// QMODE 1: a pass of that kernel that does not store (only the start value of phi is pinned, see below); 0: neither.
template <typename TL, int V, int U, bool SECOND_IS_Q, bool REF, int QMODE = 0>
__device__ __forceinline__ void scan_columns(const Levels &lv, const LevTab &lt, long long ncol, const TL *__restrict__ pt,
                                             const TL *__restrict__ pe, const double (&ps)[V], const double (&z)[V],
                                             const double (&pref)[V], int full_column, DevStatus *st, long long c2,
                                             double (&phi_ref)[V], double (&tlow)[V], int &touched,
                                             long long qdiff = 0, int l_lim = 0, bool live = false, int *low = nullptr) {
    constexpr bool STORE_Q = QMODE == 2;
    static_assert(QMODE == 0 || !SECOND_IS_Q, "the stored q is the loop pass's");
    const int N = lv.nlev;
    int lowest = N;
    // the ERA-state scan (SECOND_IS_Q) reads its rows once per file; the loop passes re-read theirs (keep those cacheable)
#define SCAN_LOADV(p, o) do { if constexpr (SECOND_IS_Q) loadv_nt<TL, V>(p, o); else loadv<TL, V>(p, o); } while (0)
    GeoAcc acc[V];
    bool mono[V];
    {
        double akN = lt.ak[N], bkN = lt.bk[N];
#pragma unroll
        for (int v = 0; v < V; ++v) {
            geo_init(acc[v], z[v], akN + ps[v] * bkN, lt.logtab);   // step_03:198
            mono[v] = ps[v] >= lv.ps_mono_min;                  // false for NaN
        }
    }
    double tn[U][V], en[U][V];
#pragma unroll
    for (int u = 0; u < U; ++u) {
        int lu = (N - 1 - u) > 0 ? (N - 1 - u) : 0;
        SCAN_LOADV(pt + (long long)lu * ncol, tn[u]);
        SCAN_LOADV(pe + (long long)lu * ncol, en[u]);
    }
#pragma unroll
    for (int v = 0; v < V; ++v) tlow[v] = tn[0][v];             // ta at the lowest full level, :303
    // phi's start value has to be IN its register here.  In k_ps_loop_multi it is the surface geopotential, which lives in
    // scratch between the passes; when its reload was still in flight at the loop's entry, its first use inside the loop
    // became an s_waitcnt vmcnt(0) in the middle of every iteration, which also waits for the rows just requested
    // (+0.09 ms per float64 file)
    if constexpr (QMODE != 0) {
#pragma unroll
        for (int v = 0; v < V; ++v) asm volatile("" : "+v"(acc[v].phi));
    }
    for (int l = N - 1; l >= 0; l -= U) {
        double t[U][V], e[U][V];
#pragma unroll
        for (int u = 0; u < U; ++u)
#pragma unroll
            for (int v = 0; v < V; ++v) { t[u][v] = tn[u][v]; e[u][v] = en[u][v]; }
        if (l - U >= 0) {
#pragma unroll
            for (int u = 0; u < U; ++u) {
                int lu = (l - U - u) > 0 ? (l - U - u) : 0;
                SCAN_LOADV(pt + (long long)lu * ncol, tn[u]);
                SCAN_LOADV(pe + (long long)lu * ncol, en[u]);
            }
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            int lc = l - u;
            if (lc >= 0) {
                double am = lt.akm[lc], bm = lt.bkm[lc], a = lt.ak[lc], b = lt.bk[lc];
                double qs[V];
#pragma unroll
                for (int v = 0; v < V; ++v) {
                    double rtv;
                    if (SECOND_IS_Q) {
                        if (REF) rtv = rd_tv_f32(t[u][v], e[u][v]);                    // float32 T, QV: float32 products
                        else rtv = CON_RD * (t[u][v] * (1 + 0.61 * e[u][v]));          // functions.py:144
                    } else {
                        // e_to_q (:196, :262-266) with the quotient formed like SharedDivisor's: reciprocal, two Newton steps,
                        // product, one residual correction - the compiler's IEEE sequence without v_div_scale / v_div_fixup
                        // (3 of its 11 instructions), the same bits for every divisor that needs no scaling (here: a pressure
                        // minus a fraction of a vapour pressure, 1e-4 .. 1.1e5 Pa)
                        const double pm = am + ps[v] * bm;
                        double q = SharedDivisor(pm - (1 - CON_MW_MD) * e[u][v]).divide(CON_MW_MD * e[u][v]);
                        rtv = CON_RD * (t[u][v] * (1 + 0.61 * q));
                        if (STORE_Q) qs[v] = q;
                    }
                    geo_layer<REF, true>(acc[v], lc, rtv, a + ps[v] * b, pref[v], lt.logtab);
                }
                if constexpr (STORE_Q) {
                    // hus_pgw is not read again by this library: streaming store
                    if (lc >= l_lim) {
                        // the row's address as the lane's own `pe` plus ONE uniform byte offset (kept opaque: re-associated into
                        // a second per-lane base it costs the two VGPRs that spill a loop-carried value, and the reload's wait).
                        // This steps from one allocation (e) into another (hus_pgw) and drops pe's const: outside what C++
                        // defines, relied on as flat global addressing of gfx950 (addresses are plain 64-bit integers); pe's
                        // __restrict__ is not violated in effect, because nothing is ever read back through the new pointer and
                        // the host refuses a hus_pgw that is one of the arrays the loop reads
                        const long long ob = (long long)lc * ncol * (long long)sizeof(TL) + qdiff;
                        const unsigned int olo = __builtin_amdgcn_readfirstlane((unsigned int)ob);
                        const unsigned int ohi = __builtin_amdgcn_readfirstlane((unsigned int)((unsigned long long)ob >> 32));
                        const long long ou = (long long)(((unsigned long long)ohi << 32) | olo);
                        if (live) storev_nt<TL, V>((TL *)((char *)const_cast<TL *>(pe) + ou), qs);
                    }
                    lowest = lc;
                }
                touched += V;
            }
        }
        if (!full_column) {
            bool above = true;
#pragma unroll
            for (int v = 0; v < V; ++v) above = above && mono[v] && (acc[v].p_lo < pref[v]) && (acc[v].kstar >= 0);
            if (__all(above)) break;
        }
    }
#pragma unroll
    for (int v = 0; v < V; ++v) phi_ref[v] = geo_finish(acc[v], pref[v], st, c2 + v);
    if constexpr (STORE_Q) *low = lowest;
}

// step_03:192-193.  REF: delta_ps is a float32 array updated in place (`delta_ps += adj_ps` casts the float64 sum back,
// step_03:182-192) and ps_pgw = PS + delta_ps is a float32 sum; the fp64 state array then holds float32 values.
template <bool REF>
__device__ __forceinline__ double next_delta_ps(double dps, double adj) { return REF ? (double)(float)(dps + adj) : dps + adj; }
template <bool REF>
__device__ __forceinline__ double ps_of(double ps0, double dps) { return REF ? (double)((float)ps0 + (float)dps) : ps0 + dps; }

template <typename T, typename TL, int V, int U, bool REF>
__global__ __launch_bounds__(BLOCK) void k_adjust_ps_step(Levels lv, int ntime, long long ncol,
                                                          const TL *__restrict__ ta, const TL *__restrict__ evap,
                                                          const T *__restrict__ PS, const T *__restrict__ FIS,
                                                          const double *__restrict__ phi_ref_era,
                                                          const double *__restrict__ dphi_clim,
                                                          double *__restrict__ delta_ps, double *__restrict__ adj_ps,
                                                          double p_ref_s, const double *__restrict__ p_ref_f,
                                                          double adj_factor, int full_column, int apply_adj,
                                                          DevStatus *st, DevStatus *clear) {
    __shared__ double s_max[BLOCK / 64];
    __shared__ unsigned int s_valid[BLOCK / 64];
    __shared__ double s_lev[LEVTAB_DOUBLES];
    if (clear && blockIdx.x == 0 && threadIdx.x == 0) {       // status block of the NEXT pass
        DevStatus z;
        z.code = 0; z.nan_seen = 0; z.col = ~0ull; z.max_bits = 0; z.valid = 0;
        z.min_targ_bits = ~0ull; z.min_src_bits = ~0ull; z.levels_touched = 0; z.qv_stored = 0;
        *clear = z;
    }
    LevTab lt = stage_levels<true, true>(lv, s_lev, BLOCK);
    long long g = (long long)blockIdx.x * BLOCK + threadIdx.x;
    long long ngroups = (long long)ntime * ncol / V;
    double amax = -1.0;       // max |err| of this thread's valid columns (-1 = none)
    int touched = 0;          // full levels read by this thread (x V columns)
    if (g < ngroups) {
        ColIdx ix = col_index(g, V, ncol);
        const int N = lv.nlev;
        long long c2 = ix.t * ncol + ix.c;
        double ps0[V], z[V], dps[V], adj[V], ps[V], pref[V], tlow[V], phi_ref[V];
        loadv<T, V>(PS + c2, ps0);
        loadv<T, V>(FIS + c2, z);
        loadv<double, V>(delta_ps + c2, dps);
        loadv<double, V>(adj_ps + c2, adj);
        if (p_ref_f) loadv<double, V>(p_ref_f + c2, pref);
        else {
#pragma unroll
            for (int v = 0; v < V; ++v) pref[v] = p_ref_s;
        }
#pragma unroll
        for (int v = 0; v < V; ++v) {
            if (apply_adj) dps[v] = next_delta_ps<REF>(dps[v], adj[v]);   // step_03:192 (already applied by k_local_p_ref otherwise)
            ps[v] = ps_of<REF>(ps0[v], dps[v]);                           // :193
        }
        if (apply_adj) storev<double, V>(delta_ps + c2, dps);
        scan_columns<TL, V, U, false, REF>(lv, lt, ncol, ta + ix.t * N * ncol + ix.c, evap + ix.t * N * ncol + ix.c, ps, z, pref,
                                           full_column, st, c2, phi_ref, tlow, touched);
        double nadj[V];
#pragma unroll
        for (int v = 0; v < V; ++v) {
            double err = (phi_ref[v] - phi_ref_era[c2 + v]) - dphi_clim[c2 + v];      // :289,298
            // :301-304.  REF: `-adj_factor * ps_pgw` is a float32 product (python float x float32 array)
            const double fps = REF ? (double)((float)(-adj_factor) * (float)ps[v]) : -adj_factor * ps[v];
            nadj[v] = fps / (CON_RD * tlow[v]) * err;
            double ae = fabs(err);
            if (ae == ae) amax = fmax(amax, ae);                                      // :308 skipna
        }
        storev<double, V>(adj_ps + c2, nadj);
    }
    // block max (exact: max is order independent) -> one atomic per block
    double wm = wave_max(amax);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) touched += __shfl_xor(touched, off, 64);
    int w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) { s_max[w] = wm; s_valid[w] = (unsigned int)touched; }
    __syncthreads();
    if (threadIdx.x == 0) {
        double m = s_max[0];
        unsigned long long tch = s_valid[0];
#pragma unroll
        for (int i = 1; i < BLOCK / 64; ++i) { m = fmax(m, s_max[i]); tch += s_valid[i]; }
        if (m >= 0.0) {
            atomicMax(&st->max_bits, dbits(m));
            atomicAdd(&st->valid, 1ull);
        }
        atomicAdd(&st->levels_touched, tch);
    }
}

// phi_ref of the ERA state from (T, QV, PS, FIS) with the hybrid pressure rebuilt in registers
// (step_03:280-287 with pa_hl_era of :64-66): no 4-D pressure array, and like the pass kernel it
// only reads the levels below p_ref.
template <typename T, int V, int U, bool REF>
__global__ __launch_bounds__(BLOCK) void k_phi_ref_hybrid(Levels lv, int ntime, long long ncol,
                                                          const T *__restrict__ ta, const T *__restrict__ hus,
                                                          const T *__restrict__ PS, const T *__restrict__ FIS,
                                                          double p_ref_s, const double *__restrict__ p_ref_f,
                                                          double *__restrict__ phi_out, int full_column, DevStatus *st) {
    __shared__ double s_lev[LEVTAB_DOUBLES];
    LevTab lt = stage_levels<true, true>(lv, s_lev, BLOCK);
    long long g = (long long)blockIdx.x * BLOCK + threadIdx.x;
    long long ngroups = (long long)ntime * ncol / V;
    if (g >= ngroups) return;
    ColIdx ix = col_index(g, V, ncol);
    const int N = lv.nlev;
    long long c2 = ix.t * ncol + ix.c;
    double ps[V], z[V], pref[V], tlow[V], phi_ref[V];
    int touched = 0;
    loadv<T, V>(PS + c2, ps);
    loadv<T, V>(FIS + c2, z);
    if (p_ref_f) loadv<double, V>(p_ref_f + c2, pref);
    else {
#pragma unroll
        for (int v = 0; v < V; ++v) pref[v] = p_ref_s;
    }
    scan_columns<T, V, U, true, REF>(lv, lt, ncol, ta + ix.t * N * ncol + ix.c, hus + ix.t * N * ncol + ix.c, ps, z, pref,
                                     full_column, st, c2, phi_ref, tlow, touched);
    storev<double, V>(phi_out + c2, phi_ref);
}

// final outputs of the loop: ps_pgw = PS + delta_ps (step_03:193,369), hus_pgw from e (:262-266,370)
// `marks` (PGW_OPT_QV_FROM_PASS, the converged pass was the storing pass of k_ps_loop_multi): per column the lowest level
// whose QV that pass has stored with this delta_ps - only the levels above it are left.  The V columns of a thread lie in
// one wave of that kernel and carry the same mark; the largest is taken all the same, and a level written twice gets the
// same bits twice.
template <typename T, typename TL, int V, bool REF>
__global__ __launch_bounds__(BLOCK) void k_finalize_ps_hus(Levels lv, int ntime, long long ncol,
                                                           const T *__restrict__ PS, const double *__restrict__ delta_ps,
                                                           const TL *__restrict__ evap, T *__restrict__ ps_out,
                                                           TL *__restrict__ hus_out, int l_start,
                                                           const unsigned short *__restrict__ marks) {
    __shared__ double s_lev[LEVTAB_DOUBLES];
    LevTab lt = stage_levels<false, true>(lv, s_lev, BLOCK);
    long long g = (long long)blockIdx.x * BLOCK + threadIdx.x;
    long long ngroups = (long long)ntime * ncol / V;
    if (g >= ngroups) return;
    ColIdx ix = col_index(g, V, ncol);
    long long c2 = ix.t * ncol + ix.c;
    double ps0[V], dps[V], ps[V];
    loadv<T, V>(PS + c2, ps0);
    loadv<double, V>(delta_ps + c2, dps);
#pragma unroll
    for (int v = 0; v < V; ++v) ps[v] = ps_of<REF>(ps0[v], dps[v]);
    if (ps_out) storev<T, V>(ps_out + c2, ps);
    if (hus_out) {
        const int N = lv.nlev;
        long long base = ix.t * N * ncol + ix.c;
        int l_end = N;
        if (marks) {
            int m = 0;
#pragma unroll
            for (int v = 0; v < V; ++v) m = marks[c2 + v] > m ? marks[c2 + v] : m;
            l_end = m < N ? m : N;
        }
        // e is read for the last time and QV is not read again by this library: streaming loads / stores
#pragma unroll 4
        for (int l = l_start; l < l_end; ++l) {        // levels < l_start were written by k_delta_quad
            double e[V], r[V];
            loadv_nt<TL, V>(evap + base + (long long)l * ncol, e);
            double am = lt.akm[l], bm = lt.bkm[l];
#pragma unroll
            for (int v = 0; v < V; ++v) r[v] = e_to_q(e[v], am + ps[v] * bm);
            storev_nt<TL, V>(hus_out + base + (long long)l * ncol, r);
        }
    }
}

// =====================================================================================
// a6  interp_logp_4d, signature-faithful                       functions.py:434-580
// Each target level is located by the reference's "first s with src[s] == x or src[s] > x" rule.  The scan
// resumes from the previous hit while targets ascend (all earlier sources are < the previous target <= x, so
// they cannot match) and restarts from 0 otherwise -> identical selection, O(N+S).
// =====================================================================================
// No field is staged (only the 2 KB table of the logarithm).  A column keeps a window of its source profile in registers - levels j-2, j-1, j (the scan
// position) and j+1, with the loads of level j+2 in flight - and moves it forward when a target passes level j, so
// every source element is read exactly once, one scan step ahead of its use, and the kernel runs at full occupancy
// (a [level][thread] LDS tile of the source columns caps the CU at 8 waves at S = 19: 0.91 vs 0.54 ms).
// A non-ascending / NaN target restarts the scan (re-reads the column from level 0; rare).
#ifndef PGW_INTERP_MINB
#define PGW_INTERP_MINB 1
#endif
#define PGW_LOGT(x) pgw_log_tab((x), s_logt)
// TV / TP / TO: storage types of var, of the two pressure fields and of the result.  One type for all three: float64
// arithmetic on the stored values.  TV = float with TO = double is the reference's dtype flow (numba, functions.py:575-578,
// as in k_hybrid_to_plev below): `src_y[i2] - src_y[i1]` is a float32 subtraction, everything else float64.
template <typename TV, typename TP, typename TO, int MODE>
__global__ __launch_bounds__(BLOCK, PGW_INTERP_MINB) void k_interp_logp_stream(int ntime, int S, int N, long long ncol,
                                                              const TV *__restrict__ var, const TP *__restrict__ srcP,
                                                              const TP *__restrict__ trgP, TO *__restrict__ out,
                                                              int logp_in, DevStatus *st) {
    constexpr bool DY32 = sizeof(TV) == 4 && sizeof(TO) == 8;
    // np.log of both pressure fields (:470-471) through the table-driven logarithm of the level loops (pgw_log_tab: ~27
    // instead of ~40 instructions, same <= 1 ulp; S + N = 156 logarithms per column made this kernel issue-bound: 0.86 busy).
    // Source and target logarithms come from the one implementation, so the exact-hit rule (:540) is unaffected.
    __shared__ double s_logt[2 * LOG_TABLE_N];
    stage_log_table(s_logt, BLOCK);
    __syncthreads();
    long long flat = (long long)blockIdx.x * BLOCK + threadIdx.x;
    if (flat >= (long long)ntime * ncol) return;
    long long t = flat / ncol, c = flat - t * ncol;
    const TV *pv = var + t * S * ncol + c;
    const TP *pp = srcP + t * S * ncol + c;
    const TP *pt = trgP + t * N * ncol + c;
    TO *po = out + t * N * ncol + c;
    const double s_first = logp_in ? (double)pp[0] : PGW_LOGT((double)pp[0]);                         // :470
    {
        double s_last = (double)pp[(long long)(S - 1) * ncol];
        if (!logp_in) s_last = PGW_LOGT(s_last);
        if (s_last < s_first) { report_ordered(st, 10, flat); }      // :500-501
        double x_first = (double)pt[0], x_last = (double)pt[(long long)(N - 1) * ncol];
        if (!logp_in) { x_first = PGW_LOGT(x_first); x_last = PGW_LOGT(x_last); }
        if (x_last < x_first) { report_ordered(st, 11, flat); }      // :502-503
    }
    // source window
    int j;
    double xmm = 0, ymm = 0, xm = 0, ym = 0, xj, yj, xn, yn, rx, ry;
    auto reset = [&]() {
        j = 0;
        xj = s_first; yj = (double)pv[0];
        xn = (double)pp[ncol]; yn = (double)pv[ncol];                // S >= 2
        if (!logp_in) xn = PGW_LOGT(xn);
        const long long o = (long long)(2 < S ? 2 : S - 1) * ncol;
        rx = (double)SIG_LD(pp + o); ry = (double)SIG_LD(pv + o);
    };
    reset();
    double xprev = -__builtin_inf();
    constexpr int U = 4;            // chunks of 4 target levels: the next chunk's loads are in flight while this one is done
    double nx[U];
#pragma unroll
    for (int u = 0; u < U; ++u) nx[u] = (double)SIG_LD(pt + (long long)(u < N ? u : N - 1) * ncol);
    for (int l0 = 0; l0 < N; l0 += U) {
        double cx[U];
#pragma unroll
        for (int u = 0; u < U; ++u) cx[u] = nx[u];
        if (l0 + U < N) {
#pragma unroll
            for (int u = 0; u < U; ++u) nx[u] = (double)SIG_LD(pt + (long long)((l0 + U + u) < N ? (l0 + U + u) : N - 1) * ncol);
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int l = l0 + u;
            if (l < N) {
                double x = cx[u];
                if (!logp_in) x = PGW_LOGT(x);                            // :471
                if (__builtin_expect(!(x >= xprev), 0)) {                // restart (descending or NaN target)
                    x = no_speculate(x);
                    reset();
                }
                while (j < S && !(xj == x || xj > x)) {                  // first s with src[s] == x or src[s] > x
                    xmm = xm; ymm = ym; xm = xj; ym = yj; xj = xn; yj = yn;
                    xn = logp_in ? rx : PGW_LOGT(rx); yn = ry;
                    ++j;
                    const long long o = (long long)(j + 2 < S ? j + 2 : S - 1) * ncol;
                    rx = (double)SIG_LD(pp + o); ry = (double)SIG_LD(pv + o);
                }
                bool extrap = false;
                double x1, y1, x2, y2;
                bool same;                                               // i1 == i2: take y1
                if (j >= S) {                                            // above range            :554-561
                    extrap = true;
                    same = (MODE != 1);
                    x1 = (MODE == 1) ? xmm : xm; y1 = (MODE == 1) ? ymm : ym; x2 = xm; y2 = ym;
                } else if (xj == x) {                                    // exact                  :540-543
                    same = true; x1 = x2 = xj; y1 = y2 = yj;
                } else if (j == 0) {                                     // below range            :530-538
                    extrap = true;
                    same = (MODE != 1);
                    x1 = xj; y1 = yj; x2 = xn; y2 = yn;
                } else {                                                 // bracket                :545-548
                    same = false; x1 = xm; y1 = ym; x2 = xj; y2 = yj;
                }
                double y;
                if (extrap && MODE == 3) y = __builtin_nan("");          // :569-570
                else if (same) y = y1;                                   // :572-573
                else if constexpr (DY32) y = y1 + (x - x1) * (double)((float)y2 - (float)y1) / (x2 - x1);
                else y = y1 + (x - x1) * (y2 - y1) / (x2 - x1);          // :575-578
                if (MODE == 0 && extrap) report_ordered(st, 12, flat);   // :564-566
                SIG_ST((TO)y, po + (long long)l * ncol);
                xprev = (x == x) ? x : __builtin_inf();                  // after a NaN target restart
            }
        }
    }
}

#undef PGW_LOGT

// =====================================================================================
// s1  hybrid model levels -> fixed pressure levels, fused      step_01_extract_deltas/CFday_interp_to_plev.py:89-134
// The source pressure of a column is ap[k] + b[k] * ps (:91; product, then sum: two roundings), formed in registers
// from ap / b staged in LDS and the column's one ps; the targets are ONE ascending list (:114) whose logarithms are
// taken once per block into LDS with the logarithm the source pressures go through (pgw_log_tab), so that the
// exact-hit rule (functions.py:540) sees equal logarithms for equal pressures.  No pressure field exists in memory:
// per column S * sizeof(TI) + sizeof(TI) bytes in, N * sizeof(TO) out, about S logarithms.
// Selection and arithmetic are interp_extrap_1d's (functions.py:511-580) as in k_interp_logp_stream above: the same
// register window (levels j-2 .. j+1 of the scan position j, the load of level j+2 in flight), the same restart for
// a target below its predecessor or NaN (only a non-monotone list takes it; the list is uniform, so a whole wave does).
// One thread owns V adjacent columns: the target loop is uniform over the wave, so each target level is one
// V-wide streaming store per lane (one coalesced segment per wave); every column keeps its own scan position, its
// source loads are per column (neighbouring lanes -> neighbouring addresses while their surface pressures are close).
// The C-ABI dispatches V = 1: the kernel is issue-bound and the second column's registers cost occupancy (pgw_capi.hip).
// src_rev / out_rev: the file's level order is surface-first (:89) / the result is wanted with pressure descending
// (:133-134) - index arithmetic on var, ap, b and on the output row, nothing is copied.
// TI = float, TO = double is the reference's dtype flow on CFday files: src_y[i2] - src_y[i1] in float32 (numba,
// functions.py:575-578), everything else float64.  TI = TO: float64 arithmetic, narrowed on the store.
// =====================================================================================
constexpr int MAX_TARG_PLEV = 256;
template <typename TI, typename TO, int V, int MODE, typename O>
__global__ __launch_bounds__(BLOCK) void k_hybrid_to_plev(int ntime, int S, int N, long long ncol,
                                                          const TI *__restrict__ var, const TI *__restrict__ ps,
                                                          const double *__restrict__ ap, const double *__restrict__ b,
                                                          const double *__restrict__ plev, int src_rev, int out_rev,
                                                          TO *__restrict__ out, DevStatus *st) {
    __shared__ double s_logt[2 * LOG_TABLE_N];
    __shared__ double s_ap[MAX_NLEV], s_b[MAX_NLEV];       // pressure ascending with the index
    __shared__ double s_lx[MAX_TARG_PLEV];                 // ln(target), :471
    // the leading levels with b = 0 (the model's pure-pressure levels, about a third of a CMIP6 model's) have the same
    // pressure ap + 0 * ps = ap in every column with a finite ps: their logarithms are taken once per block
    __shared__ double s_lap[MAX_NLEV];
    __shared__ int s_npure;
    stage_log_table(s_logt, BLOCK);
    if (threadIdx.x == 0) s_npure = S;
    for (int i = threadIdx.x; i < S; i += BLOCK) {
        const int k = src_rev ? S - 1 - i : i;
        s_ap[i] = ap[k]; s_b[i] = b[k];
    }
    __syncthreads();
    for (int i = threadIdx.x; i < N; i += BLOCK) s_lx[i] = pgw_log_tab(plev[i], s_logt);
    for (int i = threadIdx.x; i < S; i += BLOCK) {
        s_lap[i] = pgw_log_tab(s_ap[i], s_logt);
        if (!(s_b[i] == 0.0)) atomicMin(&s_npure, i);
    }
    __syncthreads();
    const int n_pure = s_npure;
    const long long g = (long long)blockIdx.x * BLOCK + threadIdx.x;
    if (g >= (long long)ntime * ncol / V) return;
    const long long flat = g * V;                          // V | ncol: a group lies within one time step
    const long long t = flat / ncol, c = flat - t * ncol;
    if (g == 0 && s_lx[N - 1] < s_lx[0]) report_ordered(st, 11, 0);       // functions.py:502-503 (the same list in every column)
    double psv[V];
    loadv<TI, V>(ps + flat, psv);
    const O rowb_in = (O)((unsigned long long)ncol * sizeof(TI)), rowb_out = (O)((unsigned long long)ncol * sizeof(TO));
    const O ov = (O)((unsigned long long)(t * S * ncol + c) * sizeof(TI));
    const O oo = (O)((unsigned long long)(t * N * ncol + c) * sizeof(TO));
    bool ps_finite[V];                                                     // 0 * ps = 0: not for NaN / inf
#pragma unroll
    for (int v = 0; v < V; ++v) ps_finite[v] = (psv[v] - psv[v] == 0.0);
    auto srcx = [&](int k, int v) {                                        // ln(ap + b * ps), :91 and functions.py:470
        const int kk = k < S ? k : S - 1;
        if (kk < n_pure && ps_finite[v]) return s_lap[kk];
        return pgw_log_tab(no_speculate(s_ap[kk] + s_b[kk] * psv[v]), s_logt);
    };
    auto ldy = [&](int k, int v) {
        const int kk = k < S ? k : S - 1;
        const int fk = src_rev ? S - 1 - kk : kk;
        return ld_off_nt<TI, O>(var, ov + (O)fk * rowb_in + (O)(v * sizeof(TI)));
    };
    int j[V];
    double xmm[V], ymm[V], xm[V], ym[V], xj[V], yj[V], xn[V], yn[V], x_first[V];
    // source levels j+2 .. j+1+H2P_DEPTH of every column: loads in flight ahead of the window.  Same box, S = 95, N = 99,
    // 2 GB in, V = 2: depth 1 / 4 / 8 = 2.83 / 2.60 / 3.11 ms for float32 in (one register per level) and 1.45 / 1.69 /
    // 2.31 ms for float64 in (two registers per level: the occupancy they cost outweighs the loads)
    constexpr int H2P_DEPTH = sizeof(TI) == 4 ? 4 : 1;
    TI ry[V][H2P_DEPTH];
#pragma unroll
    for (int v = 0; v < V; ++v) {
        x_first[v] = srcx(0, v);
        if (srcx(S - 1, v) < x_first[v]) report_ordered(st, 10, flat + v); // functions.py:500-501
    }
    auto reset = [&]() {
#pragma unroll
        for (int v = 0; v < V; ++v) {
            j[v] = 0;
            xmm[v] = ymm[v] = xm[v] = ym[v] = 0;
            xj[v] = x_first[v]; yj[v] = (double)ldy(0, v);
            xn[v] = srcx(1, v); yn[v] = (double)ldy(1, v);                 // S >= 2
#pragma unroll
            for (int d = 0; d < H2P_DEPTH; ++d) ry[v][d] = ldy(2 + d, v);
        }
    };
    reset();
    double xprev = -__builtin_inf();
    for (int l = 0; l < N; ++l) {
        double x = s_lx[l];
        if (__builtin_expect(!(x >= xprev), 0)) {                          // restart (descending or NaN target)
            x = no_speculate(x);
            reset();
        }
        double y[V];
#pragma unroll
        for (int v = 0; v < V; ++v) {
            while (j[v] < S && !(xj[v] == x || xj[v] > x)) {               // first s with src[s] == x or src[s] > x
                xmm[v] = xm[v]; ymm[v] = ym[v]; xm[v] = xj[v]; ym[v] = yj[v]; xj[v] = xn[v]; yj[v] = yn[v];
                yn[v] = (double)ry[v][0];
#pragma unroll
                for (int d = 0; d + 1 < H2P_DEPTH; ++d) ry[v][d] = ry[v][d + 1];
                ++j[v];
                xn[v] = srcx(j[v] + 1, v);
                ry[v][H2P_DEPTH - 1] = ldy(j[v] + 1 + H2P_DEPTH, v);
            }
            auto diff = [](double y2, double y1) {                         // src_y[i2] - src_y[i1], :577
                if constexpr (sizeof(TI) == 4 && sizeof(TO) == 8) return (double)((float)y2 - (float)y1);       // numba: float32 - float32
                else return y2 - y1;
            };
            // the scan stopped at the first level with src == x or src > x; 0 < j < S and src > x is the bracket (:545-548),
            // which is nearly every target: the other three cases sit behind one real branch
            if (__builtin_expect(j[v] > 0 && j[v] < S && !(xj[v] == x), 1)) {
                y[v] = ym[v] + (x - xm[v]) * diff(yj[v], ym[v]) / (xj[v] - xm[v]);                           // :575-578
            } else {
                const double xs = no_speculate(x);
                bool extrap = true, same = (MODE != 1);                    // same: i1 == i2, take y1
                double x1, y1, x2, y2;
                if (j[v] >= S) {                                           // above range            :554-561
                    x1 = (MODE == 1) ? xmm[v] : xm[v]; y1 = (MODE == 1) ? ymm[v] : ym[v]; x2 = xm[v]; y2 = ym[v];
                } else if (xj[v] == xs) {                                  // exact                  :540-543
                    extrap = false; same = true; x1 = x2 = xj[v]; y1 = y2 = yj[v];
                } else {                                                   // j == 0: below range    :530-538
                    x1 = xj[v]; y1 = yj[v]; x2 = xn[v]; y2 = yn[v];
                }
                if (extrap && MODE == 3) y[v] = __builtin_nan("");         // :569-570
                else if (same) y[v] = y1;                                  // :572-573
                else y[v] = y1 + (xs - x1) * diff(y2, y1) / (x2 - x1);     // :575-578
                if (MODE == 0 && extrap) report_ordered(st, 12, flat + v); // :564-566
            }
        }
        const O orow = oo + (O)(out_rev ? N - 1 - l : l) * rowb_out;
        storev_nt<TO, V>(reinterpret_cast<TO *>(reinterpret_cast<char *>(out) + orow), y);
        xprev = (x == x) ? x : __builtin_inf();                            // after a NaN target: restart
    }
}

// =====================================================================================
// s2  Magnus relative humidity of the Emon conversion          step_01_extract_deltas/Emon_convert_hus_to_hur.py:16-21
// RH = 0.263 * P * QV * (exp(17.67 * (T - 273.15) / (T - 29.65)))**(-1) on (time, plev, column) arrays, P the 1-D plev
// coordinate (float64).  numpy's dtype flow on float32 files: 0.263 * P is float64, so both products are float64;
// the exponent, exp and the reciprocal (x**(-1) = 1 / x) are float32.  float64 files: float64 throughout.
// =====================================================================================
template <typename T>
__global__ __launch_bounds__(BLOCK) void k_magnus_rh(long long n, int nplev, long long ncol, const T *__restrict__ qv,
                                                     const double *__restrict__ plev, const T *__restrict__ ta,
                                                     double *__restrict__ rh) {
    const long long stride = (long long)gridDim.x * BLOCK;
    for (long long i = (long long)blockIdx.x * BLOCK + threadIdx.x; i < n; i += stride) {
        const double p = plev[(i / ncol) % nplev];
        const T tk = SIG_LD(ta + i);
        const double q = (double)SIG_LD(qv + i);
        double r;
        if constexpr (sizeof(T) == 4) {
            const float a = 17.67f * (tk - 273.15f) / (tk - 29.65f);
            // pgw_expf_core is expf without its range selects: |a| < 87 covers every temperature above 36 K
            const float e = (a > -87.0f && a < 87.0f) ? pgw_expf_core(a) : expf(a);
            r = (double)(1.0f / e);
        } else {
            const double a = 17.67 * (tk - 273.15) / (tk - 29.65);
            const double e = (a > -700.0 && a < 700.0) ? pgw_exp_reduced(a) : pgw_exp(a);
            r = 1.0 / e;
        }
        SIG_ST(0.263 * p * q * r, rh + i);
    }
}

// =====================================================================================
// s3  coarse Amon hur carried onto the finer Emon levels       step_01_extract_deltas/Emon_convert_hus_to_hur.py:82-122
// Per Emon level l the host table holds either (copy = Amon index, :122) or the three Emon indices (l, the nearest
// Amon level above = lower pressure, below = higher pressure: :85-96) and the two Amon indices (:113-114).
// a = |hur_l - hur_above|, b = |hur_l - hur_below|, w_above = 1 - a / (a + b), w_below = 1 - b / (a + b),
// out = amon_above * w_above + amon_below * w_below in this order; 0 / 0 = NaN is kept.  float64 arithmetic only.
// =====================================================================================
struct MergeLevel { int copy, e_above, e_below, a_above, a_below; };       // copy >= 0: take Amon level `copy`
template <typename TA>
__global__ __launch_bounds__(BLOCK) void k_hur_merge_levels(int ntime, int nplev, int namon, long long ncol,
                                                            const double *__restrict__ hur, const TA *__restrict__ amon,
                                                            const MergeLevel *__restrict__ tab, double *__restrict__ out) {
    const long long n = (long long)ntime * nplev * ncol;
    const long long stride = (long long)gridDim.x * BLOCK;
    for (long long i = (long long)blockIdx.x * BLOCK + threadIdx.x; i < n; i += stride) {
        const long long row = i / ncol, c = i - row * ncol;
        const long long t = row / nplev;
        const int l = (int)(row - t * nplev);
        const MergeLevel m = tab[l];
        const double *h = hur + t * nplev * ncol + c;
        const TA *a = amon + t * namon * ncol + c;
        double r;
        if (m.copy >= 0) r = (double)a[(long long)m.copy * ncol];
        else {
            const double hl = h[(long long)l * ncol], ha = h[(long long)m.e_above * ncol], hb = h[(long long)m.e_below * ncol];
            const double da = fabs(hl - ha), db = fabs(hl - hb);
            const double wa = 1 - da / (da + db), wb = 1 - db / (da + db);
            r = (double)a[(long long)m.a_above * ncol] * wa + (double)a[(long long)m.a_below * ncol] * wb;
        }
        out[i] = r;
    }
}

// =====================================================================================
// s4  multi-year mean of one calendar bin      step_01_extract_deltas/extract_climate_delta.sh:153-159, 217-219, 235-238
// (`cdo ymonmean` / `cdo ydaymean` after `-selyear`: the records of one month or one day of the year, missing values
// skipped).  x (nrec, inner): the bin's records in time order, NaN = missing.  Per cell, in record order,
//   if (!isnan(x[r][i])) { sum += (double)x[r][i]; cnt += 1; }
// `first`: start from zero without reading sum / cnt; `last`: write mean = (TO)(sum / cnt) (NaN where cnt == 0, IEEE
// division) and no state.  The order of the additions IS the definition (the sequential float64 sum, bit for bit): one
// accumulator per cell, no tree.  What is unrolled is the LOADS: CLIM_UNROLL records of a cell group are in flight before
// the first of them is added.  One thread per V cells (16 B per lane), byte offsets of type O into x as in ld_off.
// =====================================================================================
constexpr int CLIM_UNROLL = 8;
template <typename T, int V, typename O>
__device__ __forceinline__ void clim_ld(const T *__restrict__ base, O byte_off, T (&out)[V]) {
    if constexpr (V == 1) out[0] = ld_off_nt<T, O>(base, byte_off);
    else {
        using VT = typename VecOf<T, V>::type;                 // V * sizeof(T) <= 16
        const VT t = ld_off_nt<VT, O>(reinterpret_cast<const VT *>(base), byte_off);
#pragma unroll
        for (int v = 0; v < V; ++v) out[v] = t[v];
    }
}
// The record walk of the kernels over x (nrec, inner): the V cells from cell i on, record after record in time order, each
// record handed to `take` as it comes; the loads of CLIM_UNROLL records are issued before the first of them is taken.
template <typename TI, int V, typename O, typename F>
__device__ __forceinline__ void clim_walk(int nrec, long long inner, const TI *__restrict__ x, long long i, F &&take) {
    const O rowb = (O)((unsigned long long)inner * sizeof(TI));
    O off = (O)((unsigned long long)i * sizeof(TI));
    int r = 0;
    for (; r + CLIM_UNROLL <= nrec; r += CLIM_UNROLL) {
        TI b[CLIM_UNROLL][V];
#pragma unroll
        for (int u = 0; u < CLIM_UNROLL; ++u) clim_ld<TI, V, O>(x, off + (O)u * rowb, b[u]);
        off += (O)CLIM_UNROLL * rowb;
#pragma unroll
        for (int u = 0; u < CLIM_UNROLL; ++u) take(b[u]);
    }
    for (; r < nrec; ++r) {
        TI b[V];
        clim_ld<TI, V, O>(x, off, b);
        off += rowb;
        take(b);
    }
}
template <typename TI, typename TO, int V, typename O>
__global__ __launch_bounds__(BLOCK) void k_clim_accumulate(int nrec, long long inner, const TI *__restrict__ x, int first,
                                                           int last, double *__restrict__ sum, int *__restrict__ cnt,
                                                           TO *__restrict__ mean) {
    static_assert(V * sizeof(TI) <= 16, "one access per record and lane");
    const long long g = (long long)blockIdx.x * BLOCK + threadIdx.x;
    if (g >= inner / V) return;                                // V | inner
    const long long i = g * V;
    double s[V];
    Pack<int, V> c;
    if (first) {
#pragma unroll
        for (int v = 0; v < V; ++v) { s[v] = 0.0; c.v[v] = 0; }
    } else {
        loadv16<double, V>(sum + i, s);
        c = *reinterpret_cast<const Pack<int, V> *>(cnt + i);
    }
    clim_walk<TI, V, O>(nrec, inner, x, i, [&](const TI (&b)[V]) {
#pragma unroll
        for (int v = 0; v < V; ++v)
            if (b[v] == b[v]) { s[v] += (double)b[v]; c.v[v] += 1; }
    });
    if (last) {
        double m[V];
#pragma unroll
        for (int v = 0; v < V; ++v) m[v] = c.v[v] > 0 ? s[v] / (double)c.v[v] : __builtin_nan("");
        storev16<TO, V>(mean + i, m);
    } else {
        storev16<double, V>(sum + i, s);
        *reinterpret_cast<Pack<int, V> *>(cnt + i) = c;
    }
}

// The loads of k_clim_accumulate and nothing else, on the same grid (diagnostic entry pgw_test_read_records: what the card
// gives this access pattern, tools/clim_time.py).  `sink` is null in every call; it keeps the loads alive.
template <typename TI, int V, typename O>
__global__ __launch_bounds__(BLOCK) void k_clim_read(int nrec, long long inner, const TI *__restrict__ x, TI *__restrict__ sink) {
    const long long g = (long long)blockIdx.x * BLOCK + threadIdx.x;
    if (g >= inner / V) return;
    TI keep[V];
#pragma unroll
    for (int v = 0; v < V; ++v) keep[v] = 0;
    clim_walk<TI, V, O>(nrec, inner, x, g * V, [&](const TI (&b)[V]) {
#pragma unroll
        for (int v = 0; v < V; ++v) keep[v] = b[v] > keep[v] ? b[v] : keep[v];
    });
    if (sink) {
#pragma unroll
        for (int v = 0; v < V; ++v) sink[g * V + v] = keep[v];
    }
}

// =====================================================================================
// p1  T_CL of a COSMO extpar file + time mean of the ts delta                     postproc_cosmo/extpar_adapt.py:20-32
//   delta_ts_clim = delta_ts.mean(dim=['time'])           xarray on a float array: np.nanmean(values, axis=0)
//   ext_file['T_CL'][:] += delta_ts_clim.values.squeeze() numpy's in-place add on netCDF4's masked array
// x (nrec, n) of TX: the records in time order, NaN = missing; base, out (n) of TB.  Per cell i:
//   1. x'[r] = isnan(x[r][i]) ? +0.0 : x[r][i];  tot = +0.0, then tot = (TX)(tot + x'[r]) for r = 0 .. nrec - 1 in record
//      order, IN TX;  cnt = number of non-NaN records.  A NaN record ADDS +0.0, and the sum starts from +0.0 (the identity
//      numpy's add.reduce starts from): 0.0 + v is v for every v but -0.0, so only a cell whose records are all -0.0 shows
//      it - its sum is +0.0, with or without a NaN record, as numpy's is.
//   2. mean = (TX)((double)tot / (double)cnt);  cnt == 0: 0 / 0 = NaN.
//   3. base[i] equal to a mask value (`mk`, already rounded to TB; a NaN mask value masks NaN cells): out[i] = base[i], bit
//      for bit.
//   4. otherwise out[i] = (TB)(base[i] + mean) with the addition in the promoted type of TB and TX; a NaN mean gives NaN.
// base == nullptr: the mean alone (out is not touched); mean == nullptr: it is not stored.  out may be base: a thread reads
// its cells before it writes them.  counts[0] += masked cells, counts[1] += unmasked cells whose base was not NaN and whose
// result is: summed over the wave, then lanes 0 and 1 add the two sums with one atomic instruction.
// The walk over the records is k_clim_accumulate's (clim_walk): one thread per V cells, one access of V * sizeof(TX) <= 16
// bytes per record and lane, byte offsets of type O into x.
// A grid of ONE cell (n == 1) is another sum in numpy: the records then lie contiguous, numpy's reduction runs along them and
// adds pairwise.  k_time_mean_add_one takes that case with numpy's order (np_pairwise_sum below); from two cells on numpy
// adds record after record, which is step 1.
// =====================================================================================
struct MeanAddMask { int n; double v[2]; };
// steps 3 and 4 for one cell: base value b, mean m -> the cell of out; the two counts are advanced
template <typename TX, typename TB>
__device__ __forceinline__ TB mean_add_cell(TB b, TX m, const MeanAddMask &mk, unsigned int &n_masked, unsigned int &n_new_nan) {
    using P = promo_t<TB, TX>;
    bool masked = false;
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const TB mv = (TB)mk.v[k];
        if (k < mk.n) masked = masked || (mv != mv ? b != b : b == mv);
    }
    const TB r = (TB)((P)b + (P)m);
    n_masked += masked ? 1u : 0u;
    n_new_nan += (!masked && b == b && r != r) ? 1u : 0u;
    return masked ? b : r;                                     // a select moves the masked cell's bits, NaN payloads included
}
template <typename TX, typename TB, int V, typename O>
__global__ __launch_bounds__(BLOCK) void k_time_mean_add(int nrec, long long n, const TB *base, MeanAddMask mk,
                                                         const TX *__restrict__ x, TB *out, TX *__restrict__ mean,
                                                         unsigned long long *__restrict__ counts) {
    static_assert(V * sizeof(TX) <= 16, "one access per record and lane");
    const long long g = (long long)blockIdx.x * BLOCK + threadIdx.x;
    unsigned int n_masked = 0, n_new_nan = 0;
    if (g < n / V) {                                           // V | n; no early return: the wave sums below need every lane
        const long long i = g * V;
        TX tot[V];
        int cnt[V];
#pragma unroll
        for (int v = 0; v < V; ++v) { tot[v] = (TX)0.0; cnt[v] = 0; }
        clim_walk<TX, V, O>(nrec, n, x, i, [&](const TX (&b)[V]) {
#pragma unroll
            for (int v = 0; v < V; ++v) {
                const bool there = b[v] == b[v];
                tot[v] = tot[v] + (there ? b[v] : (TX)0.0);
                cnt[v] += there ? 1 : 0;
            }
        });
        TX m[V];
#pragma unroll
        for (int v = 0; v < V; ++v) m[v] = (TX)((double)tot[v] / (double)cnt[v]);
        if (mean) storev_typed<TX, V>(mean + i, m);
        if (base) {
            TB b[V], o[V];
            loadv_typed<TB, V>(base + i, b);
#pragma unroll
            for (int v = 0; v < V; ++v) o[v] = mean_add_cell<TX, TB>(b[v], m[v], mk, n_masked, n_new_nan);
            storev_typed<TB, V>(out + i, o);
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        n_masked += __shfl_xor(n_masked, off, 64);
        n_new_nan += __shfl_xor(n_new_nan, off, 64);
    }
    const unsigned int lane = threadIdx.x & 63u;
    const unsigned int mine = lane == 0 ? n_masked : n_new_nan;
    if (lane < 2 && mine) atomicAdd(counts + lane, (unsigned long long)mine);
}

// numpy's pairwise_sum (numpy/core/src/umath/loops_utils.h.src) on x'[0 .. n): fewer than 8 elements are added one after the
// other from 0.0; up to 128 go into eight partial sums r[j] += x'[8 k + j], combined as ((r0 + r1) + (r2 + r3)) + ((r4 + r5) +
// (r6 + r7)), the n % 8 last ones added to that; more are split at n2 = n / 2 - (n / 2) % 8 and the halves' sums added.  The
// recursion is written with an explicit stack (depth <= log2 n).
template <typename T>
__device__ T np_block_sum(const T *__restrict__ x, long long n) {          // n <= 128
    auto at = [&](long long r) { const T v = x[r]; return v == v ? v : (T)0.0; };
    if (n < 8) {
        T res = (T)0.0;
        for (long long i = 0; i < n; ++i) res = res + at(i);
        return res;
    }
    T r[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) r[j] = at(j);
    long long i = 8;
    for (; i < n - (n % 8); i += 8) {
#pragma unroll
        for (int j = 0; j < 8; ++j) r[j] = r[j] + at(i + j);
    }
    T res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
    for (; i < n; ++i) res = res + at(i);
    return res;
}
template <typename T>
__device__ T np_pairwise_sum(const T *__restrict__ x, long long n) {
    struct Frame { long long start, len; int stage; };
    Frame st[40];
    T val[40];
    int sp = 0, nv = 0;
    st[sp++] = Frame{0, n, 0};
    while (sp > 0) {
        Frame &f = st[sp - 1];
        if (f.len <= 128) { val[nv++] = np_block_sum<T>(x + f.start, f.len); --sp; continue; }
        long long n2 = f.len / 2;
        n2 -= n2 % 8;
        if (f.stage == 0) { f.stage = 1; st[sp++] = Frame{f.start, n2, 0}; }
        else if (f.stage == 1) { f.stage = 2; st[sp++] = Frame{f.start + n2, f.len - n2, 0}; }
        else { const T right = val[--nv], left = val[--nv]; val[nv++] = left + right; --sp; }
    }
    return val[0];
}
// k_time_mean_add for a grid of one cell, one thread: tot = 0.0 + pairwise_sum(x'), then steps 2 - 4 as they are.
template <typename TX, typename TB>
__global__ void k_time_mean_add_one(int nrec, const TB *base, MeanAddMask mk, const TX *__restrict__ x, TB *out,
                                    TX *__restrict__ mean, unsigned long long *__restrict__ counts) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    int cnt = 0;
    for (int r = 0; r < nrec; ++r) cnt += x[r] == x[r] ? 1 : 0;
    const TX tot = (TX)0.0 + np_pairwise_sum<TX>(x, nrec);
    const TX m = (TX)((double)tot / (double)cnt);
    if (mean) mean[0] = m;
    if (base) {
        unsigned int n_masked = 0, n_new_nan = 0;
        out[0] = mean_add_cell<TX, TB>(base[0], m, mk, n_masked, n_new_nan);
        counts[0] = n_masked;
        counts[1] = n_new_nan;
    }
}

// =====================================================================================
// s5  difference of two climatologies (`cdo sub`)              step_01_extract_deltas/extract_climate_delta.sh:244-249
// out = (T)((double)a - (double)b) on a flat grid; NaN (missing) in either operand gives NaN.
// =====================================================================================
template <typename T, int V>
__global__ __launch_bounds__(BLOCK) void k_field_sub(long long n, const T *__restrict__ a, const T *__restrict__ b,
                                                     T *__restrict__ out) {
    const long long stride = (long long)gridDim.x * BLOCK;
    for (long long g = (long long)blockIdx.x * BLOCK + threadIdx.x; g * V < n; g += stride) {
        double x[V], y[V], r[V];
        loadv_nt<T, V>(a + g * V, x);
        loadv_nt<T, V>(b + g * V, y);
#pragma unroll
        for (int v = 0; v < V; ++v) r[v] = x[v] - y[v];
        storev_nt<T, V>(out + g * V, r);
    }
}

// =====================================================================================
// s6  level list, lon-lat box and model-top merge      step_01_extract_deltas/extract_climate_delta.sh:194-208,
//     (`cdo sellonlatbox`, `cdo sellevel`, `cdo -O merge`)      CFday_cut_subdomain.sh:28-30, Emon_add_top_from_Amon.sh:45-56
//   dst[r, lev_dst0 + k, i, j] = src[r, lev[k], lat0 + i, (lon0 + j) % nlon_src]
// A copy of words, no arithmetic: W is an unsigned word of 2, 4, 8 or 16 bytes, so NaN payloads, fill values, packed
// integers and raw big-endian file bytes go through bit for bit.  The host picks the widest W that divides the row lengths,
// lon0 (hence the place where the window wraps) and both base addresses, and hands over every longitude count in units of
// W: the wide forms ARE the scalar form on a coarser word, which is why all forms give the same bytes.
// Lanes run along the output longitude: `lpr` lanes per output row, BLOCK / lpr rows side by side in a block (a short row
// does not leave most of a wave idle), a row longer than the block is walked in steps of lpr.  Each lane takes SEL_ROWS
// rows per pass, their loads issued before the first store; blocks stride over the row tiles, so the number of rows has no
// grid limit.  The level list comes in the kernel arguments and is staged in LDS (a lane-dependent index into it).
// O: row index and byte offsets (pgw_device.h ld_off), 32-bit when source and destination are smaller than 4 GiB.
// =====================================================================================
constexpr int SEL_MAX_LEVELS = MAX_NLEV;
constexpr int SEL_ROWS = 4;                // 8 / 16 rows per lane for the 4-byte form of the example box: 0.087 / 0.074 ms against 0.075
struct SelLevels { int lev[SEL_MAX_LEVELS]; };
template <typename O> struct SelBox {
    O nrows;                               // nrec * nlev_sel * nlat_sel output rows
    unsigned int nlev_sel, nlat_sel;
    O nlev_src, nlat_src, nlon_src;        // nlon_*, lon0 in words W
    O lat0, lon0, nlon_sel;
    O nlev_dst, lev_dst0;
    unsigned int lpr, rpb;                 // lanes per row, rows per block: lpr * rpb <= BLOCK
};
template <typename W, typename O>
__global__ __launch_bounds__(BLOCK) void k_select_box(SelBox<O> a, SelLevels tab, const W *__restrict__ src, W *__restrict__ dst) {
    __shared__ int s_lev[SEL_MAX_LEVELS];
    for (unsigned int k = threadIdx.x; k < a.nlev_sel; k += BLOCK) s_lev[k] = tab.lev[k];
    __syncthreads();
    const unsigned int sub = threadIdx.x / a.lpr, lane = threadIdx.x - sub * a.lpr;
    if (sub >= a.rpb) return;                                  // BLOCK is not a multiple of lpr: the rest of the block idles
    const O tile_rows = (O)(a.rpb * SEL_ROWS);
    const O ntiles = (a.nrows + tile_rows - 1) / tile_rows;
    for (O tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        O soff[SEL_ROWS], doff[SEL_ROWS];
        bool ok[SEL_ROWS];
#pragma unroll
        for (int u = 0; u < SEL_ROWS; ++u) {
            const O row = tile * tile_rows + (O)(u * a.rpb + sub);
            ok[u] = row < a.nrows;
            const O rk = row / a.nlat_sel, i = row - rk * a.nlat_sel;
            const O r = rk / a.nlev_sel, k = rk - r * a.nlev_sel;
            const O lev = (O)s_lev[k];
            soff[u] = ((r * a.nlev_src + lev) * a.nlat_src + a.lat0 + i) * a.nlon_src * (O)sizeof(W);
            doff[u] = ((r * a.nlev_dst + a.lev_dst0 + k) * a.nlat_sel + i) * a.nlon_sel * (O)sizeof(W);
        }
        for (O j = lane; j < a.nlon_sel; j += a.lpr) {
            O js = a.lon0 + j;                                 // lon0 < nlon_src and j < nlon_sel <= nlon_src: one wrap at most
            if (js >= a.nlon_src) js -= a.nlon_src;
            W v[SEL_ROWS];
#pragma unroll
            for (int u = 0; u < SEL_ROWS; ++u)
                if (ok[u]) v[u] = ld_off_nt<W, O>(src, soff[u] + js * (O)sizeof(W));
#pragma unroll
            for (int u = 0; u < SEL_ROWS; ++u)
                if (ok[u]) st_off_nt<W, O>(dst, doff[u] + j * (O)sizeof(W), v[u]);
        }
    }
}

// =====================================================================================
// s7  lon-lat box on a curvilinear grid (`cdo sellonlatbox` on   step_01_extract_deltas/extract_climate_delta.sh:120-123,
//     the Omon / SImon tables: 2-D latitude / longitude)          194-208
// Cell (j, i) of lat / lon (nj, ni) is inside the box when both coordinates are finite, lat_lo <= lat <= lat_hi and
// lon + 360 k <= lon2 for the smallest integer k with lon + 360 k >= lon1 - k by the three lines of the host's
// `lonlat_box` (a quotient rounded up, then corrected by one either way), every operation IEEE float64 in the order written
// (contraction is off; float32 coordinates widen exactly), so numpy restates it bit for bit.
// One thread per cell, consecutive lanes along i.  An inside cell stores 1 into row_any[j] and col_any[i]: plain stores,
// several lanes may store the same 1.  n_inside: the wave's ballot is counted and lane 0 adds it with one atomic, outside
// the divergent code (no early return: the ballot needs every lane).  The entry zeroes the three outputs.
// =====================================================================================
struct BoxMark { double lon1, lon2, lat_lo, lat_hi; };
__device__ __forceinline__ bool box_inside(double lat, double lon, const BoxMark &b) {
    const double big = 1.7976931348623157e308;
    if (!(fabs(lat) <= big && fabs(lon) <= big)) return false;   // NaN and +-inf
    if (!(lat >= b.lat_lo && lat <= b.lat_hi)) return false;
    double k = ceil((b.lon1 - lon) / 360.0);
    k += (lon + 360.0 * k) < b.lon1 ? 1.0 : 0.0;
    k -= (lon + 360.0 * (k - 1.0)) >= b.lon1 ? 1.0 : 0.0;
    return lon + 360.0 * k <= b.lon2;
}
template <typename T>
__global__ __launch_bounds__(BLOCK) void k_box_mark_2d(long long n, int ni, BoxMark b, const T *__restrict__ lat,
                                                       const T *__restrict__ lon, int *__restrict__ row_any,
                                                       int *__restrict__ col_any, unsigned long long *__restrict__ n_inside) {
    const long long g = (long long)blockIdx.x * BLOCK + threadIdx.x;
    bool in = false;
    if (g < n) {
        in = box_inside((double)lat[g], (double)lon[g], b);
        if (in) {
            const long long j = g / ni;
            row_any[j] = 1;
            col_any[g - j * ni] = 1;
        }
    }
    const unsigned long long m = __ballot(in);
    if ((threadIdx.x & 63u) == 0 && m) atomicAdd(n_inside, (unsigned long long)__popcll(m));
}

// =====================================================================================
// a7  time lerp of load_delta                                  functions.py:288-292
// =====================================================================================
// TB / TA / TO: storage types of the two records and of the result.  REF (settings.function_dtype_flow = 'reference'):
// scipy's interp1d._call_linear takes `y_hi - y_lo` in the promoted type of the data - one float32 subtraction for float32
// records - slope and result in float64.
template <typename TB, int V, typename TA = TB, typename TO = TB, bool REF = false>
__global__ __launch_bounds__(BLOCK) void k_time_lerp(long long n, const TB *__restrict__ vb, const TA *__restrict__ va,
                                                     double x_hi, double x_new, TO *__restrict__ out) {
    long long stride = (long long)gridDim.x * BLOCK;
    for (long long g = (long long)blockIdx.x * BLOCK + threadIdx.x; g * V < n; g += stride) {
        double b[V], a[V], r[V];
        loadv16<TB, V>(vb + g * V, b);
        loadv16<TA, V>(va + g * V, a);
#pragma unroll
        for (int v = 0; v < V; ++v) {
            const double diff = (REF && sizeof(TB) == 4 && sizeof(TA) == 4) ? (double)((float)a[v] - (float)b[v]) : a[v] - b[v];
            r[v] = diff / x_hi * x_new + b[v];
        }
        storev16<TO, V>(out + g * V, r);
    }
}

// =====================================================================================
// a8  vert_interp_delta fused per column                        functions.py:343-431
// (+ time lerp :288-292, + era + delta step_03:170-173).  The source axis is the 1-D plev
// table (uniform, passed by value) except for the one level replace_delta_sfc moves to
// ps_hist, so nothing is staged: ln(plev) is a scalar table, delta values are gathered from
// the two bracketing records as the scan advances (each source level is read ~once).
// =====================================================================================
// The table's capacity is a compile-time property of every kernel that takes one (template parameter PT, last in each
// list, default the narrow table): the tuned kernels read it with scalar loads and stage `lnp` into an LDS array of CAP
// entries, so a kernel built for 64 entries is the same code whatever else exists.  The host picks the wide
// instantiation only for an axis of more than MAX_PLEV levels (pgw_capi.hip: with_plev).
//   MAX_PLEV       narrow table: zg's axis (k_local_p_ref, LocalPRef, pgw_geopot_on_plev) and every delta axis that fits
//   MAX_PLEV_WIDE  the cap of a delta axis (ta / hur / ua / va; the reference's step_01 writes 99 levels).  2 x 128 doubles
//                  are 2 KB of the 4 KB of kernel arguments HIP allows; a longer axis needs a table in device memory.
constexpr int MAX_PLEV = 64;
constexpr int MAX_PLEV_WIDE = 128;
template <int CAP_>
struct PlevTableT {
    static constexpr int CAP = CAP_;
    double p[CAP_];          // ascending-index order (file order reversed, :383-384)
    double lnp[CAP_];
    double pmax, pmin;
    int n;
};
using PlevTable = PlevTableT<MAX_PLEV>;
using PlevTableWide = PlevTableT<MAX_PLEV_WIDE>;
// every by-value argument of a kernel together must stay below HIP's 4 KB: asserted where a kernel takes a table
constexpr size_t KERNARG_LIMIT = 4096;
// upper bound of the argument block of a kernel with parameters A...: every argument padded to 8 bytes
template <typename... A> constexpr size_t kernarg_bytes() { return (0 + ... + ((sizeof(A) + 7) & ~(size_t)7)); }

template <typename T>
struct DeltaSrc {
    const T *b, *a;          // bracketing records (a may be null)
    double x_hi, x_new;
    // REF (reference-dtype mode): scipy's interp1d._call_linear takes y_hi - y_lo in the dtype of the file (float32 deltas:
    // one float32 subtraction), slope and result in float64 (functions.py:288-292 through xarray .interp)
    template <bool REF = false>
    __device__ __forceinline__ double get(long long off) const {
        const T rb = b[off];
        if (!a) return (double)rb;                                // :282-283
        const T ra = a[off];
        const double diff = REF ? (double)(T)(ra - rb) : (double)ra - (double)rb;
        return diff / x_hi * x_new + (double)rb;                  // :288-292 (scipy interp1d linear)
    }
    // get() addressed by byte offset (ld_off)
    template <typename O>
    __device__ __forceinline__ double get_off(O byte_off) const {
        const T rb = ld_off(b, byte_off);
        if (!a) return (double)rb;
        const T ra = ld_off(a, byte_off);
        return ((double)ra - (double)rb) / x_hi * x_new + (double)rb;
    }
    // get<REF>() of one raw record pair the caller loaded itself (all loads of a bracket change go out before the first
    // use); the division by the kernel-wide x_hi goes through a reciprocal the caller computed once (SharedDivisor: same
    // quotient bits).  `lerp` is `a != nullptr`, one property of the launch (all records of a file share the instant):
    // no per-source null test - those tests were uniform 64-bit masks kept in spilled SGPRs
    template <bool REF>
    __device__ __forceinline__ double lerp_pair(bool lerp, T rb, T ra, const SharedDivisor &by_x_hi) const {
        if (!lerp) return (double)rb;                             // :282-283
        const double diff = REF ? (double)(T)(ra - rb) : (double)ra - (double)rb;
        return by_x_hi.divide(diff) * x_new + (double)rb;         // :288-292
    }
};

// ---- rules every delta kernel follows: one statement each ------------------------------------------------------------
// The top-pressure check (functions.py:417-420) for one block: minimum target and source pressure and the NaN flags of
// its NW waves into DevStatus; the host compares the two minima.  The three LDS arrays hold one entry per wave.
template <int NW>
__device__ __forceinline__ void top_pressure_report(double min_t, double min_s, int nanflag, double (&s_mint)[NW],
                                                    double (&s_mins)[NW], int (&s_nan)[NW], DevStatus *st) {
    double wt = wave_min(min_t), ws = wave_min(min_s);
    int wn = nanflag;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) wn |= __shfl_xor(wn, off, 64);
    int w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) { s_mint[w] = wt; s_mins[w] = ws; s_nan[w] = wn; }
    __syncthreads();
    if (threadIdx.x == 0) {
        double mt = s_mint[0], ms = s_mins[0];
        int nn = s_nan[0];
        for (int i = 1; i < NW; ++i) { mt = fmin(mt, s_mint[i]); ms = fmin(ms, s_mins[i]); nn |= s_nan[i]; }
        // pressures are compared as ordered bit patterns; negative values (unphysical) map to 0
        if (mt < __builtin_inf()) atomicMin(&st->min_targ_bits, mt > 0 ? dbits(mt) : 0ull);
        if (ms < __builtin_inf()) atomicMin(&st->min_src_bits, ms > 0 ? dbits(ms) : 0ull);
        if (nn) atomicOr(&st->nan_seen, nn);
    }
}

// One table of the by-value PlevTable (p or lnp) into LDS, for lanes that index it with their own (divergent) scan
// position.  The caller synchronises afterwards.  All CAP entries of the table are copied: `lds` holds CAP doubles.
template <int CAP>
__device__ __forceinline__ void stage_plev(const double (&tab)[CAP], double *lds, int nthreads) {
    for (int i = threadIdx.x; i < CAP; i += nthreads) lds[i] = tab[i];
}

// replace_delta_sfc (functions.py:356-365) for one column: the source level `ksfc` that moves to ps_hist (-1: none) and
// whether the levels below it take the surface delta (`fill`).  A ps_hist above the file's top level is status 15 for
// column `col`; such a column inserts nothing: ksfc = -1 AND fill = false, for every caller.
// `p` is the caller's copy of the ascending pressures (an LDS array: lanes scan it with a divergent index).
// k_delta_pair and k_delta_quad keep their own text of this rule, on pt.p (uniform index: scalar loads): every form of the
// helper tried there (struct or reference results, table or scalars passed) changed the instruction counts of the tuned
// kernels' per-column preamble.  They follow the same statement, `fill` cleared included.  k_delta_pair keeps its
// source minimum too, for the same reason; k_delta_quad takes source_min (same opcode counts and registers).
// tests/test_surface_rule_edges.py holds the three texts together: ps_hist on a level, one ulp beside it, above all levels,
// on min(plev) and NaN, and NaN deltas below the ground, through every kernel that carries the rule.
struct SfcLevel { int ksfc; bool fill; };
template <typename PT, typename P>
__device__ __forceinline__ SfcLevel sfc_level(const PT &pt, const P &p, double pshv, DevStatus *st, long long col) {
    const int S = pt.n;
    SfcLevel r{-1, false};
    bool bad = false;
    if (pshv > pt.pmax) r.ksfc = S - 1;                            // :356-359
    else if (pshv < pt.pmin) bad = true;                          // :360-361
    else {                                                        // :362-365
        for (int i = 0; i < S; ++i) if (pshv > p[i]) r.ksfc = i;
        if (r.ksfc < 0) bad = true;                               // np.max of empty argwhere
        r.fill = true;
    }
    if (bad) { report(st, 15, col); r.ksfc = -1; r.fill = false; }
    return r;
}
// np.min(source_P) of the column (:417) after that insertion, folded into the lane's min_s / nanflag; `p` as above
template <bool HAS_SFC, typename P>
__device__ __forceinline__ void source_min(int S, const P &p, int ksfc, double pshv, double &min_s, int &nanflag) {
    double m = min_s;                      // folded in locals: the loop compiles to selects, as written in a kernel
    int nf = nanflag;
    for (int i = 0; i < S; ++i) {
        double v = (HAS_SFC && i == ksfc) ? pshv : p[i];
        if (v != v) nf |= 2; else m = fmin(m, v);
    }
    min_s = m;
    nanflag = nf;
}

// One variable of one column on the source axis of vert_interp_delta (functions.py:343-431): ln(plev) with level ksfc
// moved to ln(ps_hist), the delta records of the file with the surface delta at and (fill) below it; the scan position
// and the cached bracket of interp_extrap_1d ('constant', :527-578) as the caller walks its target levels.
// DY32: the reference's dtype flow takes `src_y[i2] - src_y[i1]` in float32 (numba, :575-578).
template <typename TD, bool HAS_SFC, bool DY32>
struct DeltaColumn {
    const DeltaSrc<TD> &dsrc;
    const double *s_lnp;
    const int S;
    const long long dbase, ncol;         // delta records are (ntime, S, ncol), file order
    SfcLevel sl{-1, false};
    double d_sfc = 0.0, lnps = 0.0;
    int j = 0;                           // first source index with srcx >= x
    double xprev = -__builtin_inf();
    int ci = -2;                         // cached bracket index: values y[ci], y[ci+1]
    double y_lo = 0.0, y_hi = 0.0;

    // surface insertion from (sfc, psh) of column `flat`, and with check_top the column's source minimum
    template <typename PT, typename TS, typename TH, typename P>
    __device__ __forceinline__ void insert_sfc(const PT &pt, const P &s_p, const DeltaSrc<TS> &sfc, const DeltaSrc<TH> &psh,
                                               long long flat, const double *logtab, int check_top, double &min_s,
                                               int &nanflag, DevStatus *st) {
        double pshv = 0.0;
        if (HAS_SFC) {
            pshv = psh.get(flat);
            d_sfc = sfc.get(flat);
            if constexpr (sizeof(TS) > sizeof(TD)) d_sfc = (double)(TD)d_sfc;     // stored in the delta's dtype
            sl = sfc_level(pt, s_p, pshv, st, flat);
            lnps = pgw_log_tab(pshv, logtab);
        }
        if (check_top) source_min<HAS_SFC>(S, s_p, sl.ksfc, pshv, min_s, nanflag);
    }
    __device__ __forceinline__ double srcx(int i) const { return (HAS_SFC && i == sl.ksfc) ? lnps : s_lnp[i]; }
    __device__ __forceinline__ double srcy(int i) const {
        if (HAS_SFC && sl.ksfc >= 0 && (i == sl.ksfc || (sl.fill && i > sl.ksfc))) return d_sfc;
        return dsrc.get(dbase + (long long)(S - 1 - i) * ncol);
    }
    // the delta at ln-pressure x; a descending or NaN target restarts the scan
    __device__ __forceinline__ double interp(double x) {
        if (!(x >= xprev)) j = 0;
        while (j < S) {
            double xs = srcx(j);
            if (xs == x || xs > x) break;
            ++j;
        }
        double y;
        if (j >= S) {                                   // above range, constant :558-560
            y = srcy(S - 1);
        } else {
            double xs = srcx(j);
            if (xs == x) y = srcy(j);                   // exact :540-543
            else if (j == 0) y = srcy(0);               // below range, constant :534-536
            else {
                if (ci != j - 1) { y_lo = srcy(j - 1); y_hi = srcy(j); ci = j - 1; }
                double x1 = srcx(j - 1);
                if constexpr (DY32) y = y_lo + (x - x1) * (double)((float)y_hi - (float)y_lo) / (xs - x1);
                else y = y_lo + (x - x1) * (y_hi - y_lo) / (xs - x1);    // :575-578
            }
        }
        xprev = (x == x) ? x : __builtin_inf();
        return y;
    }
};

// Storage types: TD the delta records, TP the target pressures (or `ps`), TO the result, TA the addend, TS / TH the surface
// delta and the HIST surface pressure.  One type for all: float64 arithmetic on the stored values.  TD = float with
// TO = double is the reference's dtype flow: the surface delta is stored in the delta's dtype (np.vectorize keeps it,
// functions.py:343-366), ps_hist enters the float64 source pressures, `src_y[i2] - src_y[i1]` is a float32 subtraction
// (numba, :575-578) and everything else float64.
template <typename TD, typename TP, typename TO, bool HAS_SFC, typename TA = TO, typename TS = TD, typename TH = TP, typename PT = PlevTable>
__global__ __launch_bounds__(BLOCK) void k_vert_interp_delta(PT pt, Levels lv, int ntime, int N, long long ncol,
                                                             DeltaSrc<TD> dsrc, DeltaSrc<TS> sfc, DeltaSrc<TH> psh,
                                                             const TP *__restrict__ trgP, const TP *__restrict__ ps,
                                                             int check_top, const TA *__restrict__ add_to,
                                                             TO *__restrict__ out, DevStatus *st) {
    constexpr bool DY32 = sizeof(TD) == 4 && sizeof(TO) == 8;
    static_assert(kernarg_bytes<PT, Levels, int, int, long long, DeltaSrc<TD>, DeltaSrc<TS>, DeltaSrc<TH>, void *, void *, int, void *,
                                void *, void *>() <= KERNARG_LIMIT, "kernel arguments");
    __shared__ double s_mint[BLOCK / 64], s_mins[BLOCK / 64];
    __shared__ int s_nan[BLOCK / 64];
    // plev / ln(plev) staged in LDS: lanes index them with their own (divergent) scan position
    __shared__ double s_p[PT::CAP], s_lnp[PT::CAP];
    __shared__ double s_lev[LEVTAB_DOUBLES];
    // the delta kernels take every logarithm from pgw_log_tab - like k_log_table, which makes ln(plev): the exact-hit test
    // `src_x == targ_x` (functions.py:540) compares values of ONE implementation
    LevTab lt;
    lt.akm = lt.bkm = nullptr;
    lt.logtab = s_lev + 2 * (MAX_NLEV + 1) + 2 * MAX_NLEV;
    if (!trgP) lt = stage_levels<false, true>(lv, s_lev, BLOCK);
    else stage_log_table(s_lev + 2 * (MAX_NLEV + 1) + 2 * MAX_NLEV, BLOCK);
    stage_plev(pt.p, s_p, BLOCK);
    stage_plev(pt.lnp, s_lnp, BLOCK);
    __syncthreads();
    long long flat = (long long)blockIdx.x * BLOCK + threadIdx.x;
    double min_t = __builtin_inf(), min_s = __builtin_inf();
    int nanflag = 0;
    if (flat < (long long)ntime * ncol) {
        long long t = flat / ncol, c = flat - t * ncol;
        DeltaColumn<TD, HAS_SFC, DY32> col{dsrc, s_lnp, pt.n, t * pt.n * ncol + c, ncol};
        col.insert_sfc(pt, s_p, sfc, psh, flat, lt.logtab, check_top, min_s, nanflag, st);
        double psv = 0.0;
        const TP *ptg = nullptr;
        if (trgP) ptg = trgP + t * N * ncol + c; else psv = (double)ps[flat];
        long long obase = t * N * ncol + c;
        // chunks of 4 target levels: the next chunk's target pressures and addends are in flight while this one is
        // interpolated (one memory latency per chunk instead of per level; each element is touched once: streaming forms)
        constexpr int U = 4;
        double np_[U], na_[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const long long o = (long long)(u < N ? u : N - 1) * ncol;
            np_[u] = ptg ? (double)SIG_LD(ptg + o) : 0.0;
            na_[u] = add_to ? (double)SIG_LD(add_to + obase + o) : 0.0;
        }
        for (int l0 = 0; l0 < N; l0 += U) {
        double cp_[U], ca_[U];
#pragma unroll
        for (int u = 0; u < U; ++u) { cp_[u] = np_[u]; ca_[u] = na_[u]; }
        if (l0 + U < N) {
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const long long o = (long long)((l0 + U + u) < N ? (l0 + U + u) : N - 1) * ncol;
                if (ptg) np_[u] = (double)SIG_LD(ptg + o);
                if (add_to) na_[u] = (double)SIG_LD(add_to + obase + o);
            }
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int l = l0 + u;
            if (l >= N) break;
            double p = ptg ? cp_[u] : (lt.akm[l] + psv * lt.bkm[l]);
            if (check_top) { if (p != p) nanflag |= 1; else min_t = fmin(min_t, p); }
            double y = col.interp(pgw_log_tab(p, lt.logtab));
            if (add_to) y = ca_[u] + y;                                        // step_03:170-173
            SIG_ST((TO)y, out + obase + (long long)l * ncol);
        }
        }
    }
    if (check_top) top_pressure_report<BLOCK / 64>(min_t, min_s, nanflag, s_mint, s_mins, s_nan, st);
}

// settings.i_reinterp = 1 (step_03_apply_to_era.py:202-216, 330-343), one variable, one pass, one kernel:
//   out = interp_logp_4d(era_field, pa_era, pa_pgw, 'constant')  +  load_delta_interp(var, pa_pgw)
// with both hybrid pressure fields rebuilt in registers from the two surface pressures (pa_era = akm + ps_era bkm is the
// SOURCE axis of the first term, pa_pgw = akm + ps_pgw bkm the TARGET of both), so neither 4-D pressure array nor the
// re-interpolated ERA field is materialised: reads the ERA field once, writes the result once (composed from the
// function-level entries the same work is two launches and five 4-D passes).  The ERA column is followed with a
// three-value window (level j-1, j and the raw value of j+1 in flight): the two pressure sets differ by the loop's
// surface-pressure increment, so the bracket of target level l lies next to source level l.  Selection rule and lerp
// arithmetic are interp_extrap_1d's (functions.py:527-578, 'constant'); all logarithms from pgw_log_tab.
template <typename T, bool HAS_SFC, typename PT = PlevTable>
__global__ __launch_bounds__(BLOCK) void k_reinterp_field(PT pt, Levels lv, int ntime, long long ncol,
                                                          DeltaSrc<T> dsrc, DeltaSrc<T> sfc, DeltaSrc<T> psh,
                                                          const T *__restrict__ era_field, const T *__restrict__ ps_era,
                                                          const T *__restrict__ ps_pgw, int check_top,
                                                          T *__restrict__ out, DevStatus *st) {
    static_assert(kernarg_bytes<PT, Levels, int, long long, DeltaSrc<T>, DeltaSrc<T>, DeltaSrc<T>, void *, void *, void *, int, void *,
                                void *>() <= KERNARG_LIMIT, "kernel arguments");
    __shared__ double s_mint[BLOCK / 64], s_mins[BLOCK / 64];
    __shared__ int s_nan[BLOCK / 64];
    __shared__ double s_p[PT::CAP], s_lnp[PT::CAP];
    __shared__ double s_lev[LEVTAB_DOUBLES];
    LevTab lt = stage_levels<false, true>(lv, s_lev, BLOCK);
    const int N = lv.nlev;
    stage_plev(pt.p, s_p, BLOCK);
    stage_plev(pt.lnp, s_lnp, BLOCK);
    __syncthreads();
    long long flat = (long long)blockIdx.x * BLOCK + threadIdx.x;
    double min_t = __builtin_inf(), min_s = __builtin_inf();
    int nanflag = 0;
    if (flat < (long long)ntime * ncol) {
        long long t = flat / ncol, c = flat - t * ncol;
        DeltaColumn<T, HAS_SFC, false> col{dsrc, s_lnp, pt.n, t * pt.n * ncol + c, ncol};
        col.insert_sfc(pt, s_p, sfc, psh, flat, lt.logtab, check_top, min_s, nanflag, st);
        const double pse = (double)ps_era[flat], psv = (double)ps_pgw[flat];
        const long long obase = t * (long long)N * ncol + c;
        const T *pf = era_field + obase;
        // ---- window over the ERA column: (wxm, wym) level wj - 1, (wxj, wyj) level wj, and the raw values of levels
        // wj + 1 .. wj + 4 in flight (q0..q3: the window moves one level per target level, four loads stay outstanding)
        int wj;
        double wxm = 0, wym = 0, wxj, wyj, q0, q1, q2, q3;
        auto wload = [&](int lev) -> double { return (double)SIG_LD(pf + (long long)(lev < N ? lev : N - 1) * ncol); };
        auto wreset = [&]() {
            wj = 0;
            wxj = pgw_log_tab(lt.akm[0] + pse * lt.bkm[0], lt.logtab);
            wyj = wload(0);
            q0 = wload(1); q1 = wload(2); q2 = wload(3); q3 = wload(4);
        };
        wreset();
        for (int l = 0; l < N; ++l) {
            const double p = lt.akm[l] + psv * lt.bkm[l];                                   // step_03:196-197
            if (check_top) { if (p != p) nanflag |= 1; else min_t = fmin(min_t, p); }
            const double x = pgw_log_tab(p, lt.logtab);
            if (__builtin_expect(!(x >= col.xprev), 0)) wreset();                           // descending / NaN target: both scans restart (the delta's in interp)
            // -- the ERA field at this pressure (interp_extrap_1d, 'constant')
            while (wj < N && !(wxj == x || wxj > x)) {
                wxm = wxj; wym = wyj;
                ++wj;
                if (wj < N) {
                    wxj = pgw_log_tab(lt.akm[wj] + pse * lt.bkm[wj], lt.logtab);
                    wyj = q0; q0 = q1; q1 = q2; q2 = q3;
                    q3 = wload(wj + 4);
                }
            }
            double e;
            if (wj >= N) e = wym;                                   // beyond the last source level: its value   :558-560
            else if (wxj == x || wj == 0) e = wyj;                  // exact :540-543 / before the first: its value :534-536
            else e = wym + (x - wxm) * (wyj - wym) / (wxj - wxm);   // :575-578
            // -- the climate delta at this pressure (as k_vert_interp_delta)
            const double y = col.interp(x);
            SIG_ST((T)(e + y), out + obase + (long long)l * ncol);                          // vars_era + deltas  :216
        }
    }
    if (check_top) top_pressure_report<BLOCK / 64>(min_t, min_s, nanflag, s_mint, s_mins, s_nan, st);
}

// settings.i_reinterp = 1, TWO variables that share both pressure axes in one kernel (ta + hur, whose surface insertion
// uses the same ps_hist, or ua + va): per level ONE target logarithm, one source logarithm per window step, one bracket
// search on each axis and one reciprocal per interval serve both variables (k_reinterp_field spends them per variable),
// and the delta records of a bracket are cached like k_delta_quad's (a step to the next source level fetches one level,
// not two; the constant ranges above / below the delta file's levels fetch nothing).  Quotients go through SharedDivisor
// (the compiler's own division steps: same bits as k_reinterp_field's `/` for the finite, normal-range operands here).
//
// The ERA columns are streamed with a STATIC schedule - at target level l the row of level l + 8 is requested and the
// row of level l + 4 (requested four levels earlier) is put into a per-thread LDS ring of 8 levels - and the window that
// follows the source axis reads its values from the ring by level index.  k_reinterp_field moves the window through
// registers inside its data-dependent `while` loop (value rotation q0 <- q1 <- ...): every register copy has to wait for
// the load it copies, so each level exposes a full memory latency (2 TB/s).  Here the loads are consumed by the ring
// writes in issue order with four rows in flight, and the window's `while` loop only touches LDS.  A window position the
// ring does not hold (the two surface pressures more than 3-4 levels apart, or a restart) reads global memory directly.
// T: storage type of the delta records and the surface pressures; TE0 / TE1: of the two ERA fields; TO: of the outputs.
// All equal except in reference-dtype mode on float32 files (T = float): the ERA temperature is the file's float32, RELHUM
// of the ERA state is float64 (functions.py:58-116 with a float64 pressure), and `era + delta` is float64 (step_03:209-216).
template <typename T, typename TE0 = T, typename TE1 = T, typename TO = T>
struct ReinterpPair {
    DeltaSrc<T> d[2], sfc[2];
    const TE0 *era0;
    const TE1 *era1;
    TO *out[2];
    TO *evap;              // EVAP: the vapour pressure of (out[1], out[0]) = (hur_pgw, ta_pgw), what the loop pass reads
};
constexpr int RING = 8, RING_LEAD = 4;

#ifndef RP_MINW_EVAP
#define RP_MINW_EVAP 3     // with the e_sat chain 128 VGPRs spill 116 bytes into the level loop (scratch reloads are vector loads: they drain the row prefetch)
#endif
#ifndef RP_MINW
#define RP_MINW 4
#endif
#ifndef RP_SPARE_ALL
#define RP_SPARE_ALL 0
#endif
// O: byte-offset type of ld_off / st_off (32-bit when every array is smaller than 4 GiB)
// EVAP (ta + hur inside the loop): also writes e = hur_pgw / 100 * e_sat(ta_pgw) (functions.py:123) of the STORED values,
// the iterate-independent half of relative_to_specific_humidity that k_adjust_ps_step reads - the bits of a separate
// k_humidity_hybrid<.., 2> pass over the two outputs, without reading them back
// REF (reference-dtype mode): the roundings numpy / numba put into the reference on float32 files - the record difference of
// the time interpolation in float32 (DeltaSrc::get<REF>), numba's `src_y[i2] - src_y[i1]` of interp_extrap_1d in the dtype
// of the source (float32 for an ERA field of the file, float64 for RELHUM; for the deltas float32 only when the instant is
// a record, functions.py:282-283, 575-578), everything else float64.
template <typename T, bool HAS_SFC, typename O, bool EVAP = false, typename TE0 = T, typename TE1 = T, typename TO = T, bool REF = false, typename PT = PlevTable>
__global__ __launch_bounds__(BLOCK, (EVAP ? RP_MINW_EVAP : RP_MINW)) void k_reinterp_pair(PT pt, Levels lv, int ntime, long long ncol,
                                                            ReinterpPair<T, TE0, TE1, TO> rv,
                                                            DeltaSrc<T> psh, const T *__restrict__ ps_era,
                                                            const T *__restrict__ ps_pgw, int check_top, DevStatus *st) {
    static_assert(kernarg_bytes<PT, Levels, int, long long, ReinterpPair<T, TE0, TE1, TO>, DeltaSrc<T>, void *, void *, int, void *>() <=
                  KERNARG_LIMIT, "kernel arguments");
    extern __shared__ double lds_rp[];               // akm[N] | bkm[N]
    __shared__ double s_mint[BLOCK / 64], s_mins[BLOCK / 64];
    __shared__ int s_nan[BLOCK / 64];
    __shared__ double s_p[PT::CAP], s_lnp[PT::CAP];
    __shared__ double s_logt[2 * LOG_TABLE_N];
    // slot RING: see era_at.  Not for float64 fields without `e` (RP_SPARE): that instantiation runs 4 blocks per CU, and the
    // ninth slot (2 x 2 KB) would cost it one of them.
    constexpr bool SPARE = RP_SPARE_ALL || EVAP || (sizeof(TE0) + sizeof(TE1) < 16);
    __shared__ TE0 s_ring0[RING + (SPARE ? 1 : 0)][BLOCK];
    __shared__ TE1 s_ring1[RING + (SPARE ? 1 : 0)][BLOCK];
    const int S = pt.n, N = lv.nlev;
    double *s_akm = lds_rp, *s_bkm = lds_rp + N;
    stage_log_table(s_logt, BLOCK);
    for (int i = threadIdx.x; i < N; i += BLOCK) { s_akm[i] = lv.akm[i]; s_bkm[i] = lv.bkm[i]; }
    stage_plev(pt.p, s_p, BLOCK);
    stage_plev(pt.lnp, s_lnp, BLOCK);
    __syncthreads();
    long long flat = (long long)blockIdx.x * BLOCK + threadIdx.x;
    double min_t = __builtin_inf(), min_s = __builtin_inf();
    int nanflag = 0;
    if (flat < (long long)ntime * ncol) {
        long long t = flat / ncol, c = flat - t * ncol;
        const O row = (O)((unsigned long long)ncol * sizeof(T));
        const O dbase = (O)((unsigned long long)(t * S * ncol + c) * sizeof(T));      // delta records are (ntime, S, ncol), file order
        SfcLevel sl{-1, false};                        // level moved to ps_hist
        double d_sfc0 = 0.0, d_sfc1 = 0.0, lnps = 0.0, pshv = 0.0;
        if (HAS_SFC) {
            pshv = psh.template get<REF>(flat);
            d_sfc0 = rv.sfc[0].template get<REF>(flat);
            d_sfc1 = rv.sfc[1].template get<REF>(flat);
            sl = sfc_level(pt, s_p, pshv, st, flat);
            lnps = pgw_log_tab(pshv, s_logt);
        }
        auto srcx = [&](int i) -> double { return (HAS_SFC && i == sl.ksfc) ? lnps : s_lnp[i]; };
        auto is_sfc = [&](int i) -> bool { return HAS_SFC && sl.ksfc >= 0 && (i == sl.ksfc || (sl.fill && i > sl.ksfc)); };
        if (check_top) source_min<HAS_SFC>(S, s_p, sl.ksfc, pshv, min_s, nanflag);
        // delta records of the bracket (ci, ci + 1) of both variables; all loads of a change before the first use
        int ci = -2;
        double a_lo = 0, a_hi = 0, b_lo = 0, b_hi = 0;
        const bool lerp = rv.d[0].a != nullptr;          // one instant for every record of the launch
        const SharedDivisor by_x_hi(lerp ? rv.d[0].x_hi : 1.0);
        auto tl = [&](T rb, T ra) -> double { return rv.d[0].template lerp_pair<REF>(lerp, rb, ra, by_x_hi); };
        // value differences of the column interpolations (functions.py:575-578) in the dtype numba sees them in
        auto ydiff = [&](double hi, double lo) -> double { return (REF && !lerp) ? (double)((float)hi - (float)lo) : hi - lo; };
        auto ediff0 = [](double hi, double lo) -> double { return (REF && sizeof(TE0) == 4) ? (double)((float)hi - (float)lo) : hi - lo; };
        auto ediff1 = [](double hi, double lo) -> double { return (REF && sizeof(TE1) == 4) ? (double)((float)hi - (float)lo) : hi - lo; };
        auto fetch = [&](int i1) {
            if (ci == i1) return;
            const int ih = (i1 + 1 < S) ? i1 + 1 : i1;
            const O oh = dbase + (O)(S - 1 - ih) * row, ol = dbase + (O)(S - 1 - i1) * row;
            const bool seq = (ci + 1 == i1);
            const bool need_h = !is_sfc(ih), need_l = !seq && !is_sfc(i1);
            double h0 = 0, h1 = 0, l0 = 0, l1 = 0;
            // raw records first, then the time interpolation (the quotient by the launch-wide x_hi through one reciprocal)
            T hb0 = 0, hb1 = 0, ha0 = 0, ha1 = 0, lb0 = 0, lb1 = 0, la0 = 0, la1 = 0;
            if (need_h) { hb0 = ld_off(rv.d[0].b, oh); hb1 = ld_off(rv.d[1].b, oh); if (lerp) { ha0 = ld_off(rv.d[0].a, oh); ha1 = ld_off(rv.d[1].a, oh); } }
            if (need_l) { lb0 = ld_off(rv.d[0].b, ol); lb1 = ld_off(rv.d[1].b, ol); if (lerp) { la0 = ld_off(rv.d[0].a, ol); la1 = ld_off(rv.d[1].a, ol); } }
            if (need_h) { h0 = tl(hb0, ha0); h1 = tl(hb1, ha1); }
            if (need_l) { l0 = tl(lb0, la0); l1 = tl(lb1, la1); }
            if (seq) { a_lo = a_hi; b_lo = b_hi; }
            else { a_lo = need_l ? l0 : d_sfc0; b_lo = need_l ? l1 : d_sfc1; }
            a_hi = need_h ? h0 : d_sfc0;
            b_hi = need_h ? h1 : d_sfc1;
            ci = i1;
        };
        const double pse = (double)ps_era[flat], psv = (double)ps_pgw[flat];
        // byte offsets of the level arrays in units of the first ERA field's element; the other field and the outputs scale
        // them by the ratio of the element sizes (1 unless the types differ: reference-dtype mode)
        const O erow = (O)((unsigned long long)ncol * sizeof(TE0));
        const O obase = (O)((unsigned long long)(t * (long long)N * ncol + c) * sizeof(TE0));
        static_assert(sizeof(TE1) % sizeof(TE0) == 0 && sizeof(TO) % sizeof(TE0) == 0, "element sizes");
        auto off1 = [](O o) -> O { return o * (O)(sizeof(TE1) / sizeof(TE0)); };
        auto offo = [](O o) -> O { return o * (O)(sizeof(TO) / sizeof(TE0)); };
        const TE0 *pf0 = rv.era0;
        const TE1 *pf1 = rv.era1;
        auto lev_off = [&](int lev) -> O { return obase + (O)(lev < N ? lev : N - 1) * erow; };
        // ---- the ring: at target level l it holds the ERA levels [l - 3, l + 5)
        const int tid = threadIdx.x;
        int ring_lo = 0;                                               // l - 3 (may be negative)
        // A level the ring does not hold (the two surface pressures more than 3-4 levels apart, or a restart) is fetched from
        // global memory INTO the thread's spare ring slot and read from there like any other: the window's values then never
        // depend on a vector-memory load outside this branch.  (Returned in registers, the compiler had to put
        // `s_waitcnt vmcnt(0)` at the head of the window loop - where the two paths merge - which drained the eight prefetched
        // rows and every store in flight at almost every level: 0.52 of the wave time was spent in s_waitcnt.)
        auto era_at = [&](int lev, double &u, double &v) {
            if constexpr (SPARE) {
                int slot = lev & (RING - 1);
                if (__builtin_expect(!((unsigned)(lev - ring_lo) < (unsigned)RING), 0)) {
                    const O o = lev_off(lev);
                    s_ring0[RING][tid] = ld_off(pf0, o);
                    s_ring1[RING][tid] = ld_off(pf1, off1(o));
                    slot = RING;
                }
                u = (double)s_ring0[slot][tid]; v = (double)s_ring1[slot][tid];
            } else {
                if ((unsigned)(lev - ring_lo) < (unsigned)RING) { u = (double)s_ring0[lev & (RING - 1)][tid]; v = (double)s_ring1[lev & (RING - 1)][tid]; }
                else { const O o = lev_off(lev); u = (double)ld_off(pf0, o); v = (double)ld_off(pf1, off1(o)); }
            }
        };
        TE0 na[RING_LEAD];                                              // rows in flight: levels l + 4 .. l + 7 at the top of level l
        TE1 nb[RING_LEAD];
        {
            TE0 ia[RING_LEAD];
            TE1 ib[RING_LEAD];
#pragma unroll
            for (int u = 0; u < RING_LEAD; ++u) { ia[u] = ld_off_nt(pf0, lev_off(u)); ib[u] = ld_off_nt(pf1, off1(lev_off(u))); }
#pragma unroll
            for (int u = 0; u < RING_LEAD; ++u) { na[u] = ld_off_nt(pf0, lev_off(RING_LEAD + u)); nb[u] = ld_off_nt(pf1, off1(lev_off(RING_LEAD + u))); }
#pragma unroll
            for (int u = 0; u < RING_LEAD; ++u) { s_ring0[u][tid] = ia[u]; s_ring1[u][tid] = ib[u]; }
        }
        // ---- window over the source axis: level wj - 1 (wxm, um, vm) and level wj (wxj, uj, vj)
        int wj;
        double wxm = 0, wxj, um = 0, uj, vm = 0, vj;
        auto wreset = [&]() {
            wj = 0;
            wxj = pgw_log_tab(s_akm[0] + pse * s_bkm[0], s_logt);
            era_at(0, uj, vj);
        };
        int j = 0;
        double xprev = -__builtin_inf();
        int wdiv = -1, ddiv = -2;                       // window position by_W / delta bracket by_D belong to
        SharedDivisor by_W(1.0, 1.0), by_D(1.0, 1.0);
        double dx1 = 0.0;
        for (int l0 = 0; l0 < N; l0 += RING_LEAD) {
#pragma unroll
            for (int u = 0; u < RING_LEAD; ++u) {
                const int l = l0 + u;
                if (l < N) {
                    // row l + 4 into the ring (it replaces level l - 4), row l + 8 requested
                    s_ring0[(l + RING_LEAD) & (RING - 1)][tid] = na[u];
                    s_ring1[(l + RING_LEAD) & (RING - 1)][tid] = nb[u];
                    ring_lo = l + RING_LEAD + 1 - RING;
                    { const O o = lev_off(l + 2 * RING_LEAD); na[u] = ld_off_nt(pf0, o); nb[u] = ld_off_nt(pf1, off1(o)); }
                    if (l == 0) wreset();
                    const double p = s_akm[l] + psv * s_bkm[l];                                 // step_03:196-197
                    if (check_top) { if (p != p) nanflag |= 1; else min_t = fmin(min_t, p); }
                    const double x = pgw_log_tab(p, s_logt);
                    if (__builtin_expect(!(x >= xprev), 0)) { j = 0; wreset(); wdiv = -1; }     // descending / NaN target: both scans restart
                    // -- the ERA fields at this pressure (interp_extrap_1d, 'constant')
                    while (wj < N && !(wxj == x || wxj > x)) {
                        wxm = wxj; um = uj; vm = vj;
                        ++wj;
                        if (wj < N) {
                            wxj = pgw_log_tab(s_akm[wj] + pse * s_bkm[wj], s_logt);
                            era_at(wj, uj, vj);
                        }
                    }
                    double e0, e1;
                    if (wj >= N) { e0 = um; e1 = vm; }                      // beyond the last source level: its value   :558-560
                    else if (wxj == x || wj == 0) { e0 = uj; e1 = vj; }     // exact :540-543 / before the first: its value :534-536
                    else {                                                  // :575-578
                        if (wdiv != wj) { by_W = SharedDivisor(wxj - wxm); wdiv = wj; }
                        const double dx = x - wxm;
                        e0 = um + by_W.divide(dx * ediff0(uj, um));
                        e1 = vm + by_W.divide(dx * ediff1(vj, vm));
                    }
                    // -- the climate deltas at this pressure (as k_vert_interp_delta)
                    while (j < S) {
                        double xs = srcx(j);
                        if (xs == x || xs > x) break;
                        ++j;
                    }
                    int i1, i2;
                    if (j >= S) { i1 = i2 = S - 1; }
                    else {
                        double xs = srcx(j);
                        if (xs == x) { i1 = i2 = j; }
                        else if (j == 0) { i1 = i2 = 0; }
                        else { i1 = j - 1; i2 = j; }
                    }
                    fetch(i1);
                    double y0 = a_lo, y1 = b_lo;
                    if (i1 != i2) {
                        if (ddiv != i1) { dx1 = srcx(i1); by_D = SharedDivisor(srcx(i2) - dx1); ddiv = i1; }   // once per delta bracket
                        const double x1 = dx1;
                        const double dx = x - x1;
                        y0 = a_lo + by_D.divide(dx * ydiff(a_hi, a_lo));
                        y1 = b_lo + by_D.divide(dx * ydiff(b_hi, b_lo));
                    }
                    const O o = offo(obase + (O)l * erow);
                    const TO r0 = (TO)(e0 + y0), r1 = (TO)(e1 + y1);                             // vars_era + deltas  :216
                    st_off_nt(rv.out[0], o, r0);
                    st_off_nt(rv.out[1], o, r1);
                    if (EVAP) st_off(rv.evap, o, (TO)rh_to_e((double)r1, (double)r0));
                    xprev = x;           // a NaN target leaves NaN here: the next level's `!(x >= xprev)` restarts the scans, as +inf did
                }
            }
        }
    }
    if (check_top) top_pressure_report<BLOCK / 64>(min_t, min_s, nanflag, s_mint, s_mins, s_nan, st);
}

// =====================================================================================
// Fused per-file delta kernels (production path of pgw_step03_file).
//
// k_delta_pair<THERMO=true>:  ta + hur   (step_03:91-94 RELHUM of the ERA state, functions.py:306-431
//     for both variables incl. replace_delta_sfc, step_03:170-173 add, and the iterate-independent
//     vapour pressure e = hur_pgw/100 * e_sat(ta_pgw) of functions.py:123) in ONE pass:
//     reads T, QV (+ S-level delta records), writes T_pgw and e_pgw.  RELHUM / hur_pgw are never
//     materialised (the reference deletes RELHUM before writing, step_03:373).
// k_delta_pair<THERMO=false>: ua + va    (no surface insertion): reads U, V, writes U_pgw, V_pgw.
//
// Both variables of a pair see the same target ln p and (because tas/hurs share ps_hist) the same
// modified source axis, so one log and one bracket search per level serve both.
// V adjacent columns per thread (16 B per lane); level loads are software-pipelined 2 deep.
// =====================================================================================
struct ColScan {
    int ksfc;          // source level moved to ps_hist (-1: none)
    double lnps;       // ln(ps_hist)
    int j;             // current "first source index with sx >= x"
    double xprev;
};

template <typename T>
struct PairSrc {       // the two variables of a pair
    DeltaSrc<T> a, b;
};

// Source values are gathered from global memory when a column's bracket changes and cached in registers
// (staging the S source values of every column in LDS, 304 B per column at S = 19, capped the CU at 7 waves and
// measured 25 % slower: 2.44 vs 1.85 ms).
// THERMO: 4 waves/SIMD (VGPR <= 128) with 2-level chunks measured 6 % faster than 3 waves with 4-level
// chunks (fp64-VALU/latency bound); the wind pair is HBM bound and prefers the deeper prefetch.
template <typename T, int V, bool THERMO, int U, int TPB, typename PT = PlevTable>
__global__ __launch_bounds__(TPB, THERMO ? 4 : 1) void k_delta_pair(PT pt, Levels lv, int ntime, long long ncol,
                                                    const T *__restrict__ fa, const T *__restrict__ fb,
                                                    const T *__restrict__ PS,
                                                    PairSrc<T> d3, PairSrc<T> dsfc, DeltaSrc<T> psh,
                                                    int check_top, T *__restrict__ out_a, T *__restrict__ out_b,
                                                    T *__restrict__ out_hur, DevStatus *st) {
    static_assert(kernarg_bytes<PT, Levels, int, long long, void *, void *, void *, PairSrc<T>, PairSrc<T>, DeltaSrc<T>, int, void *,
                                void *, void *, void *>() <= KERNARG_LIMIT, "kernel arguments");
    extern __shared__ double lds_pair[];            // akm[N] | bkm[N]
    __shared__ double s_mint[TPB / 64], s_mins[TPB / 64];
    __shared__ int s_nan[TPB / 64];
    __shared__ double s_lnp[PT::CAP];
    __shared__ double s_logt[2 * LOG_TABLE_N];
    const int S = pt.n;
    double *s_akm = lds_pair, *s_bkm = s_akm + lv.nlev;
    stage_log_table(s_logt, TPB);
    stage_plev(pt.lnp, s_lnp, TPB);
    for (int i = threadIdx.x; i < lv.nlev; i += TPB) {
        s_akm[i] = lv.akm[i];
        s_bkm[i] = lv.bkm[i];
    }
    __syncthreads();
    long long g = (long long)blockIdx.x * TPB + threadIdx.x;
    long long ngroups = (long long)ntime * ncol / V;
    double min_t = __builtin_inf(), min_s = __builtin_inf();
    int nanflag = 0;
    if (g < ngroups) {
        ColIdx ix = col_index(g, V, ncol);
        const int N = lv.nlev;
        long long c2 = ix.t * ncol + ix.c;
        long long dbase = ix.t * S * ncol + ix.c;     // delta records (ntime, S, ncol), file order
        long long base = ix.t * N * ncol + ix.c;
        double ps[V];
        loadv<T, V>(PS + c2, ps);
        ColScan sc[V];
        bool fillv[V];
        double sfav[V], sfbv[V];
        int ci[V];                                    // cached bracket (levels ci, ci+1)
        double ca_lo[V], ca_hi[V], cb_lo[V], cb_hi[V];
#pragma unroll
        for (int v = 0; v < V; ++v) {
            sc[v].ksfc = -1; sc[v].lnps = 0.0; sc[v].j = 0; sc[v].xprev = -__builtin_inf();
            ci[v] = -2; ca_lo[v] = ca_hi[v] = cb_lo[v] = cb_hi[v] = 0.0;
            bool fill = false;
            double sfa = 0.0, sfb = 0.0, pshv = 0.0;
            if (THERMO) {
                pshv = psh.get(c2 + v);
                sfa = dsfc.a.get(c2 + v);
                sfb = dsfc.b.get(c2 + v);
                bool bad = false;
                if (pshv > pt.pmax) sc[v].ksfc = S - 1;                        // functions.py:356-359
                else if (pshv < pt.pmin) bad = true;                          // :360-361
                else {                                                        // :362-365
                    for (int i = 0; i < S; ++i) if (pshv > pt.p[i]) sc[v].ksfc = i;     // uniform index: scalar loads
                    if (sc[v].ksfc < 0) bad = true;
                    fill = true;
                }
                if (bad) { report(st, 15, c2 + v); sc[v].ksfc = -1; fill = false; }
                sc[v].lnps = pgw_log_tab(pshv, s_logt);
            }
            fillv[v] = fill; sfav[v] = sfa; sfbv[v] = sfb;
            if (check_top) {                                                  // np.min(source_P), :417
                for (int i = 0; i < S; ++i) {
                    double p = (THERMO && i == sc[v].ksfc) ? pshv : pt.p[i];
                    if (p != p) nanflag |= 2; else min_s = fmin(min_s, p);
                }
            }
        }
        // values of source levels (i, i+1) of column v, from the register cache or global memory (ascending order i <-> file index S-1-i)
        auto fetch = [&](int v, int i1, int i2, double &a1, double &b1, double &a2, double &b2) {
            auto one = [&](int i, double &a, double &b) {
                bool sfc = THERMO && sc[v].ksfc >= 0 && (i == sc[v].ksfc || (fillv[v] && i > sc[v].ksfc));
                long long o = dbase + v + (long long)(S - 1 - i) * ncol;
                a = sfc ? sfav[v] : d3.a.get(o);
                b = sfc ? sfbv[v] : d3.b.get(o);
            };
            if (ci[v] != i1) {
                if (ci[v] + 1 == i1) { ca_lo[v] = ca_hi[v]; cb_lo[v] = cb_hi[v]; }
                else one(i1, ca_lo[v], cb_lo[v]);
                int ih = (i1 + 1 < S) ? i1 + 1 : i1;
                one(ih, ca_hi[v], cb_hi[v]);
                ci[v] = i1;
            }
            a1 = ca_lo[v]; b1 = cb_lo[v];
            if (i2 != i1) { a2 = ca_hi[v]; b2 = cb_hi[v]; } else { a2 = a1; b2 = b1; }
        };
        auto srcx = [&](int v, int i) -> double {          // unconditional LDS read + select, as in k_delta_quad
            double x = s_lnp[i]; asm("" : "+v"(x)); return (THERMO && i == sc[v].ksfc) ? sc[v].lnps : x; };
        // software pipeline: chunks of U levels; the next chunk's 2*U row loads are in flight while
        // the current chunk is processed
        double na[U][V], nb[U][V];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            int lu = u < N ? u : N - 1;
            loadv<T, V>(fa + base + (long long)lu * ncol, na[u]);
            loadv<T, V>(fb + base + (long long)lu * ncol, nb[u]);
        }
        for (int l0 = 0; l0 < N; l0 += U) {
            double ca[U][V], cb[U][V];
#pragma unroll
            for (int u = 0; u < U; ++u)
#pragma unroll
                for (int v = 0; v < V; ++v) { ca[u][v] = na[u][v]; cb[u][v] = nb[u][v]; }
            if (l0 + U < N) {
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    int lu = (l0 + U + u) < N ? (l0 + U + u) : N - 1;
                    loadv<T, V>(fa + base + (long long)lu * ncol, na[u]);
                    loadv<T, V>(fb + base + (long long)lu * ncol, nb[u]);
                }
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int l = l0 + u;
                if (l < N) {
                    double ra[V], rb[V], rh[V];
                    double am = s_akm[l], bm = s_bkm[l];
#pragma unroll
                    for (int v = 0; v < V; ++v) {
                        double pa = am + ps[v] * bm;                                   // step_03:87-88
                        if (check_top) { if (pa != pa) nanflag |= 1; else min_t = fmin(min_t, pa); }
                        double x = pgw_log_tab(pa, s_logt);                           // functions.py:471
                        ColScan &c = sc[v];
                        if (!(x >= c.xprev)) c.j = 0;
                        while (c.j < S) {
                            double xs = srcx(v, c.j);
                            if (xs == x || xs > x) break;
                            ++c.j;
                        }
                        c.xprev = (x == x) ? x : __builtin_inf();
                        // i1 == i2: single value; else bracket (i1, i2 = i1 + 1)
                        int i1, i2;
                        if (c.j >= S) { i1 = i2 = S - 1; }                            // above range, constant :558-560
                        else {
                            double xs = srcx(v, c.j);
                            if (xs == x) { i1 = i2 = c.j; }                           // exact                 :540-543
                            else if (c.j == 0) { i1 = i2 = 0; }                       // below range, constant :534-536
                            else { i1 = c.j - 1; i2 = c.j; }                          // bracket               :545-548
                        }
                        double a1, b1, a2 = 0.0, b2 = 0.0;
                        fetch(v, i1, i2, a1, b1, a2, b2);
                        double da = a1, db = b1;
                        if (i1 != i2) {                                               // :575-578
                            double x1 = srcx(v, i1), x2 = srcx(v, i2);
                            const double dx = x - x1;
                            const SharedDivisor by_Dx(x2 - x1);                       // x1 < x < x2: finite, positive
                            da = a1 + by_Dx.divide(dx * (a2 - a1));
                            db = b1 + by_Dx.divide(dx * (b2 - b1));
                        }
                        if (THERMO) {
                            double rh_era = q_to_rh(cb[u][v], pa, ca[u][v]);           // step_03:91-94
                            double ta_pgw = ca[u][v] + da;                             // step_03:170-173
                            double hur_pgw = rh_era + db;
                            ra[v] = ta_pgw;
                            rb[v] = rh_to_e(hur_pgw, ta_pgw);                          // functions.py:123
                            rh[v] = hur_pgw;
                        } else {
                            ra[v] = ca[u][v] + da;
                            rb[v] = cb[u][v] + db;
                        }
                    }
                    storev<T, V>(out_a + base + (long long)l * ncol, ra);
                    storev<T, V>(out_b + base + (long long)l * ncol, rb);
                    if (THERMO && out_hur) storev<T, V>(out_hur + base + (long long)l * ncol, rh);
                }
            }
        }
    }
    if (check_top) top_pressure_report<TPB / 64>(min_t, min_s, nanflag, s_mint, s_mins, s_nan, st);
}

// -------------------------------------------------------------------------------------
// k_delta_quad: ta + hur AND ua + va in one pass (production kernel of pgw_step03_file).
// The ta+hur pair is bound by fp64 VALU issue and leaves ~60 % of the HBM bandwidth idle; the
// ua+va pair is HBM bound and leaves the VALU mostly idle.  In one kernel the two overlap
// wave by wave (the memory pipe streams U, V while other waves compute e_sat), one ln(p) per
// level serves all four variables, and the level-loop overhead is paid once.
// Two source axes are scanned per column: the surface-modified one (ta, hur) and the plain
// plev axis (ua, va); both use the reference's "first s with sx == x or sx > x" rule.
// One column per thread, source values gathered on bracket change and cached in registers.
// -------------------------------------------------------------------------------------
#ifndef QUAD_MINW
#define QUAD_MINW 3
#endif
#ifndef QUAD_MINW_F32
#define QUAD_MINW_F32 4
#endif
// TO = storage type of the 4-D outputs.  REF (reference-dtype mode; T = float, TO = double): what numpy's promotion
// computes on float32 files - RELHUM of the ERA state through the float32 e_sat chain
// (q_to_rh_f32), float32 record differences in the time interpolation, era (float32) + delta (float64) = float64 outputs.
// streaming forms for what this kernel touches once (ERA fields in; U, V and the pure-level QV out); T_pgw and e are re-read by the loop
#define QLD ld_off_nt
#define QST st_off_nt
#define QST2 st_off
// What the kernel does for the loop when it takes the loop's first two scans along (FUSE; fixed p_ref, multi-pass loop).
// A template parameter, not an argument: the float32 instantiations (4 waves of 128 VGPRs, issue-bound) lose more in
// the level loop than the loop kernel gains - even with the scans switched off at run time - so they are built without.
// While a column is below p_ref its T, QV and then T_pgw, e are in registers, and in the loop's first pass delta_ps = 0:
// both states stand on the same half-level pressures.  So on the way up the kernel accumulates phi_ref of the ERA state
// (step_03:280-287) and of the PGW state (:196-199, 289), with scan_columns' expressions on the values the loop kernel
// would read back (T_pgw and e rounded to their storage type), and at the end does what pass 1 of k_ps_loop_multi does:
// err, adj_ps (:298-304), max |err| into the status block of pass 1, dps_hist[0] = delta_ps = 0; phi_ref_era and g * dzg
// (:292-295) are stored for the passes that follow.  Only waves whose 64 columns all have ascending half-level
// pressures (ps >= ps_mono_min; false for NaN) do this.  Any other wave sets its entry of `flags` (one byte per 64 columns)
// and leaves the loop state alone: k_ps_loop_multi<.., FLAGGED = true> then runs the loop kernel's own first scan and pass for the waves
// that hold a flagged column (both ways give the same bits).  Errors 13 / 14 of the ERA state go to `st_era`, which that
// launch folds into the status block of the file - after every error of this kernel, as when the loop kernel found them.
template <typename T>
struct FusedFirst {
    double adj_factor;
    const T *FIS;
    DeltaSrc<T> zg;
    double *phi_ref_era, *dphi_clim, *delta_ps, *adj_ps, *dps_hist;
    unsigned char *flags;
    DevStatus *st_era, *st_pass;
};

// DELTAS (k_delta_fields below): the same walk, but the four deltas themselves are the output.
template <typename T, typename TO, int U, int TPB, typename O, bool LERP, bool REF, bool FUSE, bool DELTAS = false, typename PT = PlevTable>
__global__ __launch_bounds__(TPB, (sizeof(T) == 4 || DELTAS ? QUAD_MINW_F32 : QUAD_MINW)) void k_delta_quad(PT pt, Levels lv, int ntime, long long ncol,
                                                       const T *__restrict__ fT, const T *__restrict__ fQ,
                                                       const T *__restrict__ fU, const T *__restrict__ fV,
                                                       const T *__restrict__ PS,
                                                       PairSrc<T> dth, PairSrc<T> dsfc, DeltaSrc<T> psh, PairSrc<T> dw,
                                                       int check_top, TO *__restrict__ oT, TO *__restrict__ oE,
                                                       TO *__restrict__ oHur, TO *__restrict__ oU, TO *__restrict__ oV,
                                                       TO *__restrict__ oQ, int n_pure, int n_pure_lv, DevStatus *st,
                                                       double p_ref, const FusedFirst<T> *__restrict__ ffp) {
    // FusedFirst is read from device memory where it is used (start and end of the walk): as a by-value argument its
    // 30 scalar registers were loaded at the top and lived through the level loop in spilled form (v_readlane reloads)
    // n_pure > 0: the first n_pure full levels are pure-pressure levels (bkm == 0): their pressure does not depend
    // on the surface pressure, so the final QV = e_to_q(e, akm) (step_03:262-266,370) is written here already
    // (instead of e, which only the levels below p_ref and k_finalize_ps_hus need) and the finalize kernel skips them.
    // n_pure_lv: number of leading pure-pressure levels (n_pure is 0 when the QV shortcut is off); their pressure akm[l]
    // is the same in every column, so ln(akm[l]) is taken once per block instead of once per column and level
    static_assert(!(DELTAS && FUSE), "the deltas-only instantiation has no ERA state to scan");
    // the widest argument block of the library: a table beside four record pairs (2.5 KB with the 128-entry table)
    static_assert(kernarg_bytes<PT, Levels, int, long long, void *, void *, void *, void *, void *, PairSrc<T>, PairSrc<T>, DeltaSrc<T>,
                                PairSrc<T>, int, void *, void *, void *, void *, void *, void *, int, int, void *, double, void *>() <=
                  KERNARG_LIMIT, "kernel arguments");
    extern __shared__ double lds_quad[];            // akm[N] | bkm[N] | ln(akm)[N] (first n_pure_lv entries) | ak[N+1] | bk[N+1]
    __shared__ double s_lnpref;                     // pgw_log(p_ref)
    __shared__ double s_mint[TPB / 64], s_mins[TPB / 64];
    __shared__ int s_nan[TPB / 64];
    __shared__ double s_lnp[PT::CAP];
    __shared__ double s_logt[2 * LOG_TABLE_N];      // table of pgw_log_tab: every logarithm of the delta kernels (see k_vert_interp_delta)
    const int S = pt.n;
    double *s_akm = lds_quad, *s_bkm = lds_quad + lv.nlev, *s_lnpa = lds_quad + 2 * lv.nlev;
    double *s_ak = lds_quad + 3 * lv.nlev, *s_bk = s_ak + lv.nlev + 1;
    stage_log_table(s_logt, TPB);
    stage_plev(pt.lnp, s_lnp, TPB);
    for (int i = threadIdx.x; i < lv.nlev; i += TPB) { s_akm[i] = lv.akm[i]; s_bkm[i] = lv.bkm[i]; }
    if (FUSE) {
        for (int i = threadIdx.x; i <= lv.nlev; i += TPB) { s_ak[i] = lv.ak[i]; s_bk[i] = lv.bk[i]; }
        if (threadIdx.x == 0) s_lnpref = pgw_log(p_ref);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < n_pure_lv; i += TPB) s_lnpa[i] = pgw_log_tab(s_akm[i], s_logt);
    __syncthreads();
    long long flat = (long long)blockIdx.x * TPB + threadIdx.x;
    double min_t = __builtin_inf(), min_s = __builtin_inf();
    int nanflag = 0;
    bool fuse_wave = false;
    double abs_err = -1.0;                          // |err| of pass 1 in this column (FusedFirst); -1: none
    // every delta record of a file is interpolated to the same instant: ONE (x_hi, x_new) pair and one reciprocal
    // instead of the seven copies in the argument structs (28 SGPRs; the kernel was spilling scalars to VGPR lanes)
    const double x_hi = dth.a.x_hi, x_new = dth.a.x_new;
    const SharedDivisor by_x_hi(x_hi);                      // unused (a == nullptr) when the instant is a record
    const DeltaSrc<T> sTa{dth.a.b, dth.a.a, x_hi, x_new}, sHur{dth.b.b, dth.b.a, x_hi, x_new};
    const DeltaSrc<T> sUa{dw.a.b, dw.a.a, x_hi, x_new}, sVa{dw.b.b, dw.b.a, x_hi, x_new};
    if (flat < (long long)ntime * ncol) {
        const int N = lv.nlev;
        long long t = flat / ncol, c = flat - t * ncol;
        // byte offsets (type O, see ld_off): delta records (ntime, S, ncol), fields (ntime, N, ncol)
        const O row = (O)((unsigned long long)ncol * sizeof(T));
        const O dbase = (O)((unsigned long long)(t * S * ncol + c) * sizeof(T));
        const O base = (O)((unsigned long long)(t * N * ncol + c) * sizeof(T));
        const O orow = (O)((unsigned long long)ncol * sizeof(TO));          // outputs: their own element size
        const O obase = (O)((unsigned long long)(t * N * ncol + c) * sizeof(TO));
        const double ps = (double)PS[flat];
        const bool ps_finite = __builtin_fabs(ps) <= 1.7976931348623157e308;   // false for NaN, +-inf
        // ---- surface insertion for ta / hur (replace_delta_sfc, functions.py:343-366)
        int ksfc = -1;
        bool fill = false;
        double pshv = psh.template get<REF>(flat), sfa = dsfc.a.template get<REF>(flat), sfb = dsfc.b.template get<REF>(flat);
        {
            bool bad = false;
            if (pshv > pt.pmax) ksfc = S - 1;                                  // :356-359
            else if (pshv < pt.pmin) bad = true;                              // :360-361
            else {                                                            // :362-365
                for (int i = 0; i < S; ++i) if (pshv > pt.p[i]) ksfc = i;
                if (ksfc < 0) bad = true;
                fill = true;
            }
            if (bad) { report(st, 15, flat); ksfc = -1; fill = false; }
        }
        const double lnps = pgw_log_tab(pshv, s_logt);
        if (check_top) source_min<true>(S, pt.p, ksfc, pshv, min_s, nanflag);
        // modified axis: unconditional LDS read + select (the compiler otherwise wraps the read in a divergent branch;
        // the empty asm keeps the load where it is; 8 of 82 exec-mask regions of the loop gone, 2.28 -> 2.25 ms)
        auto sx1 = [&](int i) -> double { double v = s_lnp[i]; asm("" : "+v"(v)); return (i == ksfc) ? lnps : v; };
        auto is_sfc = [&](int i) -> bool { return ksfc >= 0 && (i == ksfc || (fill && i > ksfc)); };
        // register caches: source levels (ci, ci+1) of each pair
        int ci1 = -2, ci2 = -2;
        double a_lo = 0, a_hi = 0, b_lo = 0, b_hi = 0;       // ta, hur
        double c_lo = 0, c_hi = 0, d_lo = 0, d_hi = 0;       // ua, va
        // A bracket change gathers the records of the new source level(s) from global memory.  All loads of one change are
        // issued back to back BEFORE the first use (raw values into registers, then the time interpolation): one exposed
        // memory latency per change instead of one per value (the first version waited after every record pair - 2 to 4
        // serial round trips per change, the largest part of the kernel's 0.51 s_waitcnt share).
        auto tl = [&](const DeltaSrc<T> &sv, T rb, T ra) -> double { return sv.template lerp_pair<REF>(LERP, rb, ra, by_x_hi); };
        auto off_of = [&](int i) -> O { return dbase + (O)(S - 1 - i) * row; };
        auto fetch1 = [&](int i1) {
            if (ci1 == i1) return;
            const int ih = (i1 + 1 < S) ? i1 + 1 : i1;
            const O oh = off_of(ih);
            const bool seq = (ci1 - 1 == i1);
            const O o = off_of(i1);
            T lb0 = ld_off(sTa.b, o), lb1 = ld_off(sHur.b, o), la0 = 0, la1 = 0, hb0 = 0, hb1 = 0, ha0 = 0, ha1 = 0;
            if (LERP) { la0 = ld_off(sTa.a, o); la1 = ld_off(sHur.a, o); }
            if (!seq) {
                hb0 = ld_off(sTa.b, oh); hb1 = ld_off(sHur.b, oh);
                if (LERP) { ha0 = ld_off(sTa.a, oh); ha1 = ld_off(sHur.a, oh); }
            }
            if (seq) { a_hi = a_lo; b_hi = b_lo; }
            else { a_hi = is_sfc(ih) ? sfa : tl(sTa, hb0, ha0); b_hi = is_sfc(ih) ? sfb : tl(sHur, hb1, ha1); }
            a_lo = is_sfc(i1) ? sfa : tl(sTa, lb0, la0);
            b_lo = is_sfc(i1) ? sfb : tl(sHur, lb1, la1);
            ci1 = i1;
        };
        // plain-axis bracket (ci2, ci2 + 1): its lower abscissa and the reciprocal of its ln-pressure interval, taken when the
        // bracket changes instead of at every level (2 LDS reads, v_rcp_f64 and 4 FMAs per level less: 1.60 -> 1.55 ms same
        // box).  float32 storage only: the float64 instantiation sits at its 3-wave register budget (164 of 168 VGPRs; with
        // the six more live registers it spills) and its time is its bytes.
        double px1 = 0.0;
        SharedDivisor by_Dp(1.0, 1.0);
        constexpr bool HOIST_DP = (sizeof(T) == 4) || DELTAS;     // DELTAS holds no prefetched rows: room for every storage type
        auto plain_bracket = [&](int i1, int ih) { if (HOIST_DP) { px1 = s_lnp[i1]; by_Dp = SharedDivisor(s_lnp[ih] - px1); } };
        auto fetch2 = [&](int i1) {
            if (ci2 == i1) return;
            const int ih = (i1 + 1 < S) ? i1 + 1 : i1;
            const O oh = off_of(ih);
            const bool seq = (ci2 - 1 == i1);
            plain_bracket(i1, ih);
            const O o = off_of(i1);
            T lb0 = ld_off(sUa.b, o), lb1 = ld_off(sVa.b, o), la0 = 0, la1 = 0, hb0 = 0, hb1 = 0, ha0 = 0, ha1 = 0;
            if (LERP) { la0 = ld_off(sUa.a, o); la1 = ld_off(sVa.a, o); }
            if (!seq) {
                hb0 = ld_off(sUa.b, oh); hb1 = ld_off(sVa.b, oh);
                if (LERP) { ha0 = ld_off(sUa.a, oh); ha1 = ld_off(sVa.a, oh); }
            }
            if (seq) { c_hi = c_lo; d_hi = d_lo; }
            else { c_hi = tl(sUa, hb0, ha0); d_hi = tl(sVa, hb1, ha1); }
            c_lo = tl(sUa, lb0, la0);
            d_lo = tl(sVa, lb1, la1);
            ci2 = i1;
        };
        // both axes step down to the same bracket (they coincide above the surface insertion): the records of all four
        // variables in one batch
        auto fetch12 = [&](int i1) {
            if (!(ci1 - 1 == i1 && ci2 - 1 == i1)) { fetch2(i1); fetch1(i1); return; }
            const O o = off_of(i1);
            T b0 = ld_off(sTa.b, o), b1 = ld_off(sHur.b, o), b2 = ld_off(sUa.b, o), b3 = ld_off(sVa.b, o);
            T a0 = 0, a1 = 0, a2 = 0, a3 = 0;
            if (LERP) { a0 = ld_off(sTa.a, o); a1 = ld_off(sHur.a, o); a2 = ld_off(sUa.a, o); a3 = ld_off(sVa.a, o); }
            plain_bracket(i1, i1 + 1);
            a_hi = a_lo; b_hi = b_lo; c_hi = c_lo; d_hi = d_lo;
            a_lo = is_sfc(i1) ? sfa : tl(sTa, b0, a0);
            b_lo = is_sfc(i1) ? sfb : tl(sHur, b1, a1);
            c_lo = tl(sUa, b2, a2);
            d_lo = tl(sVa, b3, a3);
            ci1 = ci2 = i1;
        };
        // y_hi - y_lo of the column interpolation (functions.py:575-578): numba takes it in the delta's dtype - float64
        // after a time interpolation, the file's float32 when the instant is a record (REF && !LERP)
        auto ydiff = [](double hi, double lo) -> double {
            return (REF && !LERP) ? (double)((float)hi - (float)lo) : hi - lo; };
        // the column is walked from the surface up: targets descend, both scans start above the last source level and
        // step down while the level below them still satisfies the reference's rule (`src == x or src > x`)
        int j1 = S, j2 = S;
        double xprev = __builtin_inf();
        // ---- the loop's first two scans (FusedFirst): wave-uniform switches, the accumulators of this lane's column
        fuse_wave = FUSE && __all(ps >= lv.ps_mono_min);
        if (FUSE && (threadIdx.x & 63) == 0) ffp->flags[flat >> 6] = fuse_wave ? 0 : 1;
        bool below_pref = fuse_wave;                  // some column of the wave has not passed p_ref yet
        GeoMono<2> geo{{0.0, 0.0}, {0.0, 0.0}, 0.0, 0.0, false};          // [0] ERA state, [1] PGW state of pass 1
        if (FUSE && fuse_wave) geo_mono_init(geo, (double)ffp->FIS[flat], s_ak[N] + ps * s_bk[N], s_logt);          // step_03:198
        // ---- level loop from the surface up, chunks of U levels with the next chunk's 4*U rows in flight
        T nT[U], nQ[U], nU[U], nV[U];                 // prefetched rows stay in the storage type until they are used
#pragma unroll
        for (int u = 0; u < U; ++u) {
            O o = base + (O)((N - 1 - u) > 0 ? (N - 1 - u) : 0) * row;
            if constexpr (!DELTAS) { nT[u] = QLD(fT, o); nQ[u] = QLD(fQ, o); nU[u] = QLD(fU, o); nV[u] = QLD(fV, o); }
        }
        for (int l0 = N - 1; l0 >= 0; l0 -= U) {
            T cT[U], cQ[U], cU[U], cV[U];
#pragma unroll
            for (int u = 0; u < U; ++u) if constexpr (!DELTAS) { cT[u] = nT[u]; cQ[u] = nQ[u]; cU[u] = nU[u]; cV[u] = nV[u]; }
            if (!DELTAS && l0 - U >= 0) {
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    O o = base + (O)((l0 - U - u) > 0 ? (l0 - U - u) : 0) * row;
                    nT[u] = QLD(fT, o); nQ[u] = QLD(fQ, o); nU[u] = QLD(fU, o); nV[u] = QLD(fV, o);
                }
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int l = l0 - u;
                if (l >= 0) {
                    double pa = s_akm[l] + ps * s_bkm[l];                          // step_03:87-88
                    if (check_top) { if (pa != pa) nanflag |= 1; else min_t = fmin(min_t, pa); }
                    double x;                                                      // functions.py:471
                    if (l < n_pure_lv) x = ps_finite ? s_lnpa[l] : pa;             // pa == akm[l]; NaN for a non-finite ps
                    else x = pgw_log_tab(pa, s_logt);
                    if (!(x <= xprev)) { j1 = S; j2 = S; }
                    while (j2 > 0) { double xs = s_lnp[j2 - 1]; if (!(xs == x || xs > x)) break; --j2; }
                    xprev = x;           // a NaN target leaves NaN here: the next level's `!(x <= xprev)` restarts the scans, as -inf did
                    // ua, va on the plain plev axis
                    double dc, dd;
                    int p1, p2;                                                    // its bracket
                    if (j2 >= S) { p1 = p2 = S - 1; }                              // above range, constant :558-560
                    else {
                        double xs = s_lnp[j2];
                        if (xs == x) { p1 = p2 = j2; }                             // exact                 :540-543
                        else if (j2 == 0) { p1 = p2 = 0; }                         // below range, constant :534-536
                        else { p1 = j2 - 1; p2 = j2; }                             // bracket               :545-548
                    }
                    const bool same_axis = (ksfc < 0 || j2 < ksfc);       // ta / hur stand at the same bracket (see below)
                    if (same_axis) fetch12(p1); else fetch2(p1);
                    dc = c_lo; dd = d_lo;
                    double dxp = 0.0;
                    if (p1 != p2) {                                                // :575-578
                        if (HOIST_DP) dxp = x - px1;
                        else {
                            double x1 = s_lnp[p1], x2 = s_lnp[p2];
                            dxp = x - x1;
                            by_Dp = SharedDivisor(x2 - x1);                        // x1 < x < x2: finite, positive
                        }
                        dc = c_lo + by_Dp.divide(dxp * ydiff(c_hi, c_lo));
                        dd = d_lo + by_Dp.divide(dxp * ydiff(d_hi, d_lo));
                    }
                    // ta, hur on the axis modified by the surface insertion (level ksfc moved to ps_hist, :362-365).
                    // Source levels below index ksfc are untouched, so while the plain scan stands at j2 < ksfc the
                    // modified scan stands there too (same values, same rule): same bracket, same x - x1, same divisor.
                    double da, db;
                    if (same_axis) {
                        da = a_lo; db = b_lo;
                        if (p1 != p2) {
                            da = a_lo + by_Dp.divide(dxp * ydiff(a_hi, a_lo));
                            db = b_lo + by_Dp.divide(dxp * ydiff(b_hi, b_lo));
                        }
                    } else {
                        // j1 only moves here: at and below the surface insertion, where the walk starts
                        while (j1 > 0) { double xs = sx1(j1 - 1); if (!(xs == x || xs > x)) break; --j1; }
                        int i1, i2;
                        if (j1 >= S) { i1 = i2 = S - 1; }
                        else {
                            double xs = sx1(j1);
                            if (xs == x) { i1 = i2 = j1; }
                            else if (j1 == 0) { i1 = i2 = 0; }
                            else { i1 = j1 - 1; i2 = j1; }
                        }
                        fetch1(i1);
                        da = a_lo; db = b_lo;
                        if (i1 != i2) {
                            double x1 = sx1(i1), x2 = sx1(i2);
                            const double dx = x - x1;
                            const SharedDivisor by_Dx(x2 - x1);
                            da = a_lo + by_Dx.divide(dx * ydiff(a_hi, a_lo));
                            db = b_lo + by_Dx.divide(dx * ydiff(b_hi, b_lo));
                        }
                    }
                    const O o = obase + (O)l * orow;
                    if constexpr (DELTAS) {                                        // functions.py:472-473: float64 rows
                        QST(oT, o, (TO)da); QST(oHur, o, (TO)db); QST(oU, o, (TO)dc); QST(oV, o, (TO)dd);
                    } else {
                        QST(oU, o, (TO)((double)cU[u] + dc));                                  // step_03:170-173
                        QST(oV, o, (TO)((double)cV[u] + dd));
                        double rh_era;                                                 // step_03:91-94
                        if (REF) rh_era = q_to_rh_f32((float)cQ[u], pa, (float)cT[u]);
                        else rh_era = q_to_rh((double)cQ[u], pa, (double)cT[u]);
                        double ta_pgw = (double)cT[u] + da;
                        double hur_pgw = rh_era + db;
                        QST2(oT, o, (TO)ta_pgw);
                        double e_pgw = rh_to_e(hur_pgw, ta_pgw);                       // functions.py:123
                        if (l < n_pure) QST(oQ, o, (TO)e_to_q_ns(e_pgw, pa));          // pa == akm[l] for every finite ps
                        else QST2(oE, o, (TO)e_pgw);
                        if (oHur) st_off(oHur, o, (TO)hur_pgw);
                        if (FUSE && below_pref) {                                      // layer l of both scans, as in scan_columns
                            double rtv[2];
                            if (REF) rtv[0] = rd_tv_f32((double)cT[u], (double)cQ[u]);
                            else rtv[0] = CON_RD * ((double)cT[u] * (1 + 0.61 * (double)cQ[u]));   // functions.py:144
                            const double tp = (double)(TO)ta_pgw, ep = (double)(TO)e_pgw;          // what the loop kernel reads back
                            const double q = SharedDivisor(pa - (1 - CON_MW_MD) * ep).divide(CON_MW_MD * ep);   // e_to_q, ps_of(ps, 0) == ps
                            rtv[1] = CON_RD * (tp * (1 + 0.61 * q));
                            geo_mono_layer<REF>(geo, rtv, s_ak[l] + ps * s_bk[l], p_ref, s_lnpref, s_logt);
                            below_pref = !__all(geo.p_lo < p_ref && geo.have);      // scan_columns' stop, level by level
                        }
                    }
                }
            }
        }
        if (FUSE && fuse_wave) {                                                   // pass k = 0 of k_ps_loop_multi
            const FusedFirst<T> ff = *ffp;
            const double phi_era = geo_mono_finish(geo, 0, p_ref, ff.st_era, flat);
            const double phi_pgw = geo_mono_finish(geo, 1, p_ref, ff.st_pass, flat);
            double dphi;
            if (REF && !ff.zg.a) dphi = (double)((float)ff.zg.b[flat] * (float)CON_G);                    // see k_dphi_clim
            else dphi = ff.zg.template get<REF>(flat) * CON_G;                                            // step_03:292-295
            const double tlow = (double)ld_off(oT, obase + (O)(N - 1) * orow);     // T_pgw of the lowest level as stored above, :303
            const double err = (phi_pgw - phi_era) - dphi;                         // :289,298
            const double fps = REF ? (double)((float)(-ff.adj_factor) * (float)ps) : -ff.adj_factor * ps;
            const double ae = fabs(err);
            if (ae == ae) abs_err = ae;                                            // :308 skipna
            ff.phi_ref_era[flat] = phi_era;
            ff.dphi_clim[flat] = dphi;
            ff.dps_hist[flat] = 0.0;                                               // next_delta_ps(0, 0), :182-184,192
            ff.delta_ps[flat] = 0.0;
            ff.adj_ps[flat] = fps / (CON_RD * tlow) * err;                         // :301-304
        }
    }
    if (FUSE) {                                        // all lanes of the wave meet here (wave_max shuffles)
        const double wm = wave_max(abs_err);
        if ((threadIdx.x & 63) == 0 && wm >= 0.0) { DevStatus *sp = ffp->st_pass; atomicMax(&sp->max_bits, dbits(wm)); atomicAdd(&sp->valid, 1ull); }
    }
    if (check_top) top_pressure_report<TPB / 64>(min_t, min_s, nanflag, s_mint, s_mins, s_nan, st);
}

// -------------------------------------------------------------------------------------
// k_delta_fields: the four deltas k_delta_quad adds, as arrays (step_03 --debug_mode interpolate_full, step_03:350-361:
// the reference writes what load_delta_interp returned, functions.py:306-340).  It is k_delta_quad<.., DELTAS = true>:
// the quad kernel's own body with everything around the delta walk compiled out - no ERA field is read (fT, fQ, fU, fV
// unused), no humidity chain, no loop scans - so era + delta in numpy gives production's bits.  Inputs: the surface
// pressure the levels stand on (PS of the file; the converged ps_pgw under i_reinterp, step_03:212-216, 336-343) and the
// record gathers; outputs: four streaming float64 rows per level in oT, oHur, oU, oV (xr.zeros_like(targ_P),
// functions.py:472-473: float64 on float32 files too; oE, oQ unused).  With no prefetched rows to hold, the level loop is
// not chunked (U = 1), four waves fit for every storage type and the plain-axis bracket's reciprocal is hoisted for all.
// -------------------------------------------------------------------------------------
template <typename T, typename O, bool LERP, bool REF, typename PT = PlevTable>
constexpr auto k_delta_fields = k_delta_quad<T, double, 1, 128, O, LERP, REF, false, true, PT>;

// =====================================================================================
// a10  bilinear regridding (lat then lon)                      functions.py:817-893
// =====================================================================================
template <typename T>
__global__ __launch_bounds__(BLOCK) void k_zonal_mean_rows(long long nfield, int nlat_s, int nlon_s,
                                                           const T *__restrict__ src, int south_row, int north_row,
                                                           double *__restrict__ pole /* [nfield][2] */) {
    // one wave per (field, pole); NaN-skipping mean like xarray .mean(dim=lon) (:836,:841).
    // Sequential pairwise-free summation order differs from numpy's pairwise sum by O(eps).
    long long wv = ((long long)blockIdx.x * BLOCK + threadIdx.x) >> 6;
    int lane = threadIdx.x & 63;
    if (wv >= nfield * 2) return;
    long long f = wv >> 1;
    int which = (int)(wv & 1);
    int row = which ? north_row : south_row;
    if (row < 0) return;
    const T *r = src + (f * nlat_s + row) * nlon_s;
    double sum = 0.0;
    long long cnt = 0;
    for (int i = lane; i < nlon_s; i += 64) {
        double v = (double)r[i];
        if (v == v) { sum += v; cnt += 1; }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        sum += __shfl_xor(sum, off, 64);
        cnt += __shfl_xor(cnt, off, 64);
    }
    if (lane == 0) pole[f * 2 + which] = cnt > 0 ? sum / (double)cnt : __builtin_nan("");
}

struct RegridTables {
    const int *lat_lo, *lat_hi, *lat_oob;
    const double *lat_dx, *lat_Dx;
    const int *lon_lo, *lon_hi, *lon_oob;
    const double *lon_dx, *lon_Dx;
};

// A block owns 256 * W consecutive target longitudes of one target latitude row (W = 2 where the row length allows:
// each thread then stores two adjacent values per plane as one 16-B store - the kernel is write-dominated, 1.89 of its
// 2.03 GB, and 8-B-per-lane stores reached 3.4 TB/s where the 16-B kernels of this library reach 5.5-6) and walks the
// fields (time x plev planes).  All its points interpolate between the same two source rows, and 512 target longitudes
// of a 0.25 deg grid fall on ~140 consecutive source columns, so per plane the block first does the LATITUDE pass once
// per needed source column (coalesced loads of the two source rows; the values the reference's first interp1d produces
// at those columns, :859) into LDS, and each thread then takes its neighbours from LDS for the LONGITUDE pass (:892) -
// instead of four uncoalesced 8-byte gathers per output, which kept the texture-address path, not HBM, busy
// (2.4 TB/s).  Arithmetic per output value is unchanged: slope*(x_new-x_lo)+y_lo as scipy interp1d, twice.
// Source columns are addressed relative to the first valid lane's lower neighbour, modulo nlon_s (periodic
// wrap); a block whose points span more than REGRID_SPAN source columns (coarse or unsorted targets) gathers
// directly like the first version.  FU planes per step; the next step's source loads are issued before this
// step's stores.
constexpr int REGRID_SPAN = BLOCK;       // one source column per thread

// TOUT: the element type of `out` where it is not the source's (a float32 delta file under a float64 ERA5 file and the other
// way round, DeltaSet records regridded on the device): every value is rounded to T first - what the regridded FILE would
// hold - and that T value converted to TOUT - what the host's astype makes of the file.  float -> double is exact, double ->
// float one rounding.  TOUT = T is the kernel as it was.
template <typename T, int FU, int W, typename TOUT = T>
__global__ __launch_bounds__(BLOCK) void k_regrid(long long nfield, int nlat_s, int nlon_s, int nlat_t, int nlon_t,
                                                  unsigned int bx, unsigned int gz, const T *__restrict__ src, RegridTables tb,
                                                  const double *__restrict__ pole, TOUT *__restrict__ out) {
    __shared__ double s_y[FU][REGRID_SPAN];
    __shared__ int s_first, s_span;
    // 1-D grid of bx * nlat_t * gz blocks.  Blocks b and b + 8 run on the same XCD (MI355X_MICROARCH.md, workgroup
    // dispatch), each XCD with its own L2: with gz a multiple of 8, XCD group b % 8 takes the z-slices g, g + 8, ... so
    // a source plane is fetched into ONE L2 instead of all eight, and the blocks resident on an XCD together are
    // neighbours in (x, j) of the same planes.  Speed only; any placement is correct.
    int bxi, j, bz;
    {
        const unsigned int L = blockIdx.x, per_slice = bx * (unsigned int)nlat_t;
        unsigned int w = L, g = 0;
        if (gz % 8 == 0) { g = L & 7u; w = L >> 3; }
        const unsigned int sub = w / per_slice, rem = w - sub * per_slice;
        bz = (gz % 8 == 0) ? (int)(sub * 8u + g) : (int)sub;
        j = (int)(rem / bx);                                    // target lat
        bxi = (int)(rem - (unsigned int)j * bx);
    }
    const int i0 = (bxi * BLOCK + threadIdx.x) * W;             // first target lon of this thread (W | nlon_t when W > 1)
    const bool active = i0 < nlon_t;
    const int jl = tb.lat_lo[j], jh = tb.lat_hi[j];
    const double ldx = tb.lat_dx[j], lDx = tb.lat_Dx[j];
    const bool lat_oob = tb.lat_oob[j] != 0;
    int il[W], ih[W];
    double odx[W], oDx[W];
    bool oob[W], valid[W];
#pragma unroll
    for (int w = 0; w < W; ++w) {
        const int ii = active ? i0 + w : nlon_t - 1;
        il[w] = tb.lon_lo[ii]; ih[w] = tb.lon_hi[ii];
        odx[w] = tb.lon_dx[ii]; oDx[w] = tb.lon_Dx[ii];
        oob[w] = lat_oob || tb.lon_oob[ii];
        valid[w] = active && !tb.lon_oob[ii];
    }
    const long long plane_s = (long long)nlat_s * nlon_s, plane_t = (long long)nlat_t * nlon_t;
    const bool lo_pole = jl < 0 || jl >= nlat_s, hi_pole = jh < 0 || jh >= nlat_s;
    const long long row_lo = (long long)(lo_pole ? 0 : jl) * nlon_s, row_hi = (long long)(hi_pole ? 0 : jh) * nlon_s;
    const int lo_which = jl < 0 ? 0 : 1, hi_which = jh < 0 ? 0 : 1;
    // the grid spacings divide every plane's differences: reciprocals once per thread (SharedDivisor).  lDx == 0 (the
    // reference's pole row beside a source row at -90 itself): the reciprocal and with it every quotient is NaN, where the
    // reference has slope = +-inf or NaN times x_new - x_lo = 0: NaN too (tests/test_regrid_edges_hip.py, `pole in source`)
    const SharedDivisor by_lDx(lDx);
    struct DivW { SharedDivisor d[W]; };
    const DivW by_o = [&]() { if constexpr (W == 1) return DivW{{SharedDivisor(oDx[0])}}; else return DivW{{SharedDivisor(oDx[0]), SharedDivisor(oDx[1])}}; }();
    const SharedDivisor (&by_oDx)[W] = by_o.d;
    // source-column window of this block: starts at the lower neighbour of the first valid target
    if (threadIdx.x == 0) { s_first = BLOCK * W; s_span = 0; }
    __syncthreads();
#pragma unroll
    for (int w = 0; w < W; ++w) if (valid[w]) atomicMin(&s_first, (int)threadIdx.x * W + w);
    __syncthreads();
    const int first = s_first;                            // BLOCK * W if the block has no valid point
    int c0 = 0;
    if (first < BLOCK * W) c0 = tb.lon_lo[bxi * BLOCK * W + first];
    int rl[W], rh[W];
#pragma unroll
    for (int w = 0; w < W; ++w) {
        rl[w] = il[w] - c0; rh[w] = ih[w] - c0;
        if (rl[w] < 0) rl[w] += nlon_s;
        if (rh[w] < 0) rh[w] += nlon_s;
        if (valid[w]) atomicMax(&s_span, (rl[w] > rh[w] ? rl[w] : rh[w]) + 1);
    }
    __syncthreads();
    const int span = s_span;
    const bool staged = !lat_oob && span <= REGRID_SPAN;
    // fields of this z-slice
    long long per = (nfield + gz - 1) / gz;
    long long f0 = (long long)bz * per, f1 = f0 + per < nfield ? f0 + per : nfield;
    TOUT *po = out + (long long)j * nlon_t + (active ? i0 : 0);
    auto store = [&](long long f, const double (&r)[W]) {
        // W * sizeof(TOUT) aligned: W | nlon_t, W | i0 and `out` itself (the host picks W); streaming: the output must not
        // push the source planes out of L2
        if constexpr (std::is_same<T, TOUT>::value) storev_nt<T, W>(po + f * plane_t, r);
        else {
            double rt[W];
#pragma unroll
            for (int w = 0; w < W; ++w) rt[w] = (double)(T)r[w];
            storev_nt<TOUT, W>(po + f * plane_t, rt);
        }
    };
    if (staged) {
        // this thread's source column of the window (threads >= span idle in the latitude pass)
        const bool loader = (int)threadIdx.x < span;
        int col = c0 + (int)threadIdx.x;
        if (col >= nlon_s) col -= nlon_s;
        if (!loader) col = 0;
        int li[W], hi[W];
#pragma unroll
        for (int w = 0; w < W; ++w) { li[w] = valid[w] ? rl[w] : 0; hi[w] = valid[w] ? rh[w] : 0; }
        double v_lo[FU], v_hi[FU];
        auto fetch = [&](long long f) {                    // the two source rows of FU planes at this thread's column
#pragma unroll
            for (int u = 0; u < FU; ++u) {
                long long ff = (f + u < f1) ? f + u : f1 - 1;
                const T *sp = src + ff * plane_s;
                v_lo[u] = lo_pole ? pole[ff * 2 + lo_which] : (double)sp[row_lo + col];
                v_hi[u] = hi_pole ? pole[ff * 2 + hi_which] : (double)sp[row_hi + col];
            }
        };
        if (loader && f0 < f1) fetch(f0);
        for (long long f = f0; f < f1; f += FU) {
            if (loader) {
#pragma unroll
                for (int u = 0; u < FU; ++u) s_y[u][threadIdx.x] = by_lDx.divide(v_hi[u] - v_lo[u]) * ldx + v_lo[u];   // lat pass :859
            }
            __syncthreads();
            if (loader && f + FU < f1) fetch(f + FU);      // next planes' loads fly during this group's stores
            double ya[FU][W], yb[FU][W];
#pragma unroll
            for (int u = 0; u < FU; ++u)
#pragma unroll
                for (int w = 0; w < W; ++w) { ya[u][w] = s_y[u][li[w]]; yb[u][w] = s_y[u][hi[w]]; }
            __syncthreads();                               // s_y is rewritten by the next group of planes
            if (active) {
#pragma unroll
                for (int u = 0; u < FU; ++u) {
                    if (f + u < f1) {
                        double r[W];
#pragma unroll
                        for (int w = 0; w < W; ++w)
                            r[w] = oob[w] ? __builtin_nan("") : by_oDx[w].divide(yb[u][w] - ya[u][w]) * odx[w] + ya[u][w];   // lon pass :892
                        store(f + u, r);
                    }
                }
            }
        }
        return;
    }
    // window wider than the tile (target coarser than the source, unsorted target longitudes) or latitude out of
    // bounds: four direct gathers per point, like the first version of this kernel
    for (long long f = f0; f < f1; f += FU) {
        double ya[FU][W], yb[FU][W];
#pragma unroll
        for (int u = 0; u < FU; ++u) {
            long long ff = (f + u < f1) ? f + u : f1 - 1;
            const T *sp = src + ff * plane_s;
#pragma unroll
            for (int w = 0; w < W; ++w) {
                double a_lo = 0, b_lo = 0, a_hi = 0, b_hi = 0;
                if (!oob[w]) {
                    a_lo = lo_pole ? pole[ff * 2 + lo_which] : (double)sp[row_lo + il[w]];
                    b_lo = lo_pole ? pole[ff * 2 + lo_which] : (double)sp[row_lo + ih[w]];
                    a_hi = hi_pole ? pole[ff * 2 + hi_which] : (double)sp[row_hi + il[w]];
                    b_hi = hi_pole ? pole[ff * 2 + hi_which] : (double)sp[row_hi + ih[w]];
                }
                ya[u][w] = by_lDx.divide(a_hi - a_lo) * ldx + a_lo;                      // lat pass at the lower lon  :859
                yb[u][w] = by_lDx.divide(b_hi - b_lo) * ldx + b_lo;                      // lat pass at the upper lon
            }
        }
        if (active) {
#pragma unroll
            for (int u = 0; u < FU; ++u) {
                if (f + u < f1) {
                    double r[W];
#pragma unroll
                    for (int w = 0; w < W; ++w)
                        r[w] = oob[w] ? __builtin_nan("") : by_oDx[w].divide(yb[u][w] - ya[u][w]) * odx[w] + ya[u][w];   // lon pass  :892
                    store(f + u, r);
                }
            }
        }
    }
}

// a10, point-wise targets: `ds_gcm.interp({lat: targ_lat}).interp({lon: targ_lon})` (functions.py:859, :892) with 2-D
// targ_lat / targ_lon over shared dimensions (a rotated-pole extpar file, an unstructured cell list) is xarray's point-wise
// interpolation - every target g has its own latitude bracket as well as its own longitude bracket.  Per target and plane,
// the arithmetic of k_regrid (same order, same scale-free quotients: the same bits where the target is a mesh):
//   ya = (v[hi_row, lon_lo] - v[lo_row, lon_lo]) / lat_Dx * lat_dx + v[lo_row, lon_lo]      lat pass at the lower column
//   yb = the same at lon_hi;   out = (yb - ya) / lon_Dx * lon_dx + ya                        lon pass
// row -1 / nlat_s is the pole value of k_zonal_mean_rows; oob gives NaN.  A thread owns ONE flat target, keeps its four
// corners, the two dx and the two reciprocals in registers and walks the planes of its z-slice (blockIdx.y) with streaming
// stores; the next plane's four gathers are issued before this plane's store.  A corner is kept as one int: >= 0 an
// element of the plane, -1 / -2 the south / north pole value.  A target that is oob or past the end reads element 0 and
// is not used.  Two things the first version had were measured and removed (same bits in every form):
// staging the bounding box of a block's entries in LDS never beat gathering - neighbouring targets gather from the same few
// cache lines of a source plane that stays in L2, and the staging added a barrier per plane; and with it gone, 2 / 4 targets
// per lane (16-byte stores, 114 / 162 VGPRs) were slower than this form (52-56 VGPRs, 8 waves): the gathers, not the
// stores, bound the kernel.
struct PointTables {
    const int *lat_lo, *lat_hi, *lon_lo, *lon_hi, *oob;
    const double *lat_dx, *lat_Dx, *lon_dx, *lon_Dx;
};

// TOUT as in k_regrid: the value is rounded to T - what pgw_regrid_points stores - and that T value converted to TOUT
// (`regrid_points(x).astype(out)`); TOUT = T is the kernel as it was.
template <typename T, typename TOUT = T>
__global__ __launch_bounds__(BLOCK) void k_regrid_points(long long nfield, int nlat_s, int nlon_s, long long ntarg, unsigned int gz,
                                                         const T *__restrict__ src, PointTables tb, const double *__restrict__ pole,
                                                         TOUT *__restrict__ out) {
    const long long g0 = (long long)blockIdx.x * BLOCK + threadIdx.x;
    const bool active = g0 < ntarg;
    const long long g = active ? g0 : ntarg - 1;
    const bool oob = tb.oob[g] != 0;
    const bool live = active && !oob;
    const int jl = tb.lat_lo[g], jh = tb.lat_hi[g], il = tb.lon_lo[g], ih = tb.lon_hi[g];
    const double ldx = tb.lat_dx[g], odx = tb.lon_dx[g];
    // reciprocals once per target (SharedDivisor); a Dx of 0 gives NaN like k_regrid's
    const SharedDivisor by_lDx(tb.lat_Dx[g]), by_oDx(tb.lon_Dx[g]);
    int c[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int row = k < 2 ? jl : jh;
        int code = row * nlon_s + ((k & 1) ? ih : il);
        if (row < 0) code = -1;
        if (row >= nlat_s) code = -2;
        c[k] = live ? code : 0;
    }
    const long long plane_s = (long long)nlat_s * nlon_s;
    const long long per = (nfield + gz - 1) / gz;
    const long long f0 = (long long)blockIdx.y * per, f1 = f0 + per < nfield ? f0 + per : nfield;
    auto gather = [&](long long f, T (&v)[4]) {
        const T *sp = src + f * plane_s;
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] = sp[c[k] >= 0 ? c[k] : 0];
    };
    T cur[4], nxt[4];
    if (f0 < f1) gather(f0, cur);
    for (long long f = f0; f < f1; ++f) {
        if (f + 1 < f1) gather(f + 1, nxt);                   // the next plane's loads fly during this plane's store
        double v[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] = c[k] >= 0 ? (double)cur[k] : pole[f * 2 + (-1 - c[k])];
        const double ya = by_lDx.divide(v[2] - v[0]) * ldx + v[0];                // lat pass at the lower lon  :859
        const double yb = by_lDx.divide(v[3] - v[1]) * ldx + v[1];                // lat pass at the upper lon
        const double r = oob ? __builtin_nan("") : by_oDx.divide(yb - ya) * odx + ya;   // lon pass  :892
        if (active) __builtin_nontemporal_store((TOUT)(T)r, out + f * ntarg + g0);   // streaming: the output must not push the source planes out of L2
        if (f + 1 < f1) {
#pragma unroll
            for (int k = 0; k < 4; ++k) cur[k] = nxt[k];
        }
    }
}

// =====================================================================================
// a10w  wind components on a rotated-pole target grid (not in the reference: its targets are lat-lon meshes)
// A file on a `rotated_latitude_longitude` mapping stores U along increasing rlon and V along increasing rlat; the GCM's
// ua / va are eastward / northward.  At a target at geographic (lat, lon) [deg], north pole of the rotated grid at
// (pole_lat, pole_lon) [deg] (COSMO's uv2uvrot):
//   D  = pole_lon - lon
//   a1 = cos(pole_lat) sin(D)
//   a2 = sin(pole_lat) cos(lat) - cos(pole_lat) sin(lat) cos(D)
//   rho = sqrt(a1^2 + a2^2)           (the cosine of the target's rotated latitude)
//   c = a2 / rho,  s = a1 / rho;      u_rot = u c - v s,  v_rot = u s + v c;      inverse: u = u_rot c + v_rot s, v = -u_rot s + v_rot c
// rho == 0 (a pole of the rotated grid: no direction) gives (c, s) = (1, 0); a NaN coordinate gives NaN.
// =====================================================================================
// sin and cos of an angle in degrees, exact at the multiples of 90 (a pole at 90 N has cos = 0 and the rotation is the
// identity, where cos(pi / 2) is 6e-17): the angle less its nearest multiple of 90 - an exact difference - goes through
// sincos in radians (x * (pi / 180), numpy's deg2rad) and the quadrant turns the pair.  NaN and infinities give NaN.
__device__ __forceinline__ void sincos_deg(double x, double &s, double &c) {
    const double k = rint(x / 90.0);
    double sr, cr;
    sincos((x - 90.0 * k) * (M_PI / 180.0), &sr, &cr);
    const double m = fmod(k, 4.0);
    const int q = (m == m) ? ((int)m + 4) & 3 : 0;
    s = q == 0 ? sr : q == 1 ? cr : q == 2 ? -sr : -cr;
    c = q == 0 ? cr : q == 1 ? -sr : q == 2 ? -cr : sr;
}

// one target per lane
__global__ __launch_bounds__(BLOCK) void k_wind_rotation(long long n, const double *__restrict__ lat, const double *__restrict__ lon,
                                                         double pole_lat, double pole_lon, double *__restrict__ cos_out,
                                                         double *__restrict__ sin_out) {
    const long long g = (long long)blockIdx.x * BLOCK + threadIdx.x;
    if (g >= n) return;
    double sp, cp, sl, cl, sd, cd;
    sincos_deg(pole_lat, sp, cp);
    sincos_deg(lat[g], sl, cl);
    sincos_deg(pole_lon - lon[g], sd, cd);
    const double a1 = cp * sd;
    const double a2 = sp * cl - cp * sl * cd;
    const double rho = sqrt(a1 * a1 + a2 * a2);
    cos_out[g] = rho == 0.0 ? 1.0 : a2 / rho;
    sin_out[g] = rho == 0.0 ? 0.0 : a1 / rho;
}

// The rotation of one value pair by a target's (c, s) in float64, each result rounded once to T; `s` comes negated for
// the inverse (u c - v (-s) is u c + v s, u (-s) + v c is -u s + v c: numpy's bits).
template <typename T>
__device__ __forceinline__ void rotate_uv(double u, double v, double c, double s, T &u_rot, T &v_rot) {
    u_rot = (T)(u * c - v * s);
    v_rot = (T)(u * s + v * c);
}

// u, v (nfield, n) -> u_out, v_out (nfield, n), in place when u_out == u and v_out == v (no __restrict__ on the four: a
// lane stores a plane's elements after it has read them, and reads and stores nobody else's).  A lane owns V consecutive
// targets - 16 bytes of T per access where n and the addresses allow, V = 1 otherwise: the same arithmetic per element, the
// same bits - keeps their c and s in registers and walks the planes of its z-slice (blockIdx.y) like k_regrid_points: the
// next plane's two loads are issued before this plane's two streaming stores.
template <typename T, int V>
__global__ __launch_bounds__(BLOCK) void k_rotate_pair(long long nfield, long long n, unsigned int gz, const T *u, const T *v,
                                                       const double *__restrict__ cs, const double *__restrict__ sn, int inverse,
                                                       T *u_out, T *v_out) {
    const long long g = ((long long)blockIdx.x * BLOCK + threadIdx.x) * V;
    if (g >= n) return;
    double c[V], s[V];
    loadv16<double, V>(cs + g, c);
    loadv16<double, V>(sn + g, s);
    if (inverse) {
#pragma unroll
        for (int i = 0; i < V; ++i) s[i] = -s[i];
    }
    const long long per = (nfield + gz - 1) / gz;
    const long long f0 = (long long)blockIdx.y * per, f1 = f0 + per < nfield ? f0 + per : nfield;
    double cu[V], cv[V], nu[V], nv[V];
    if (f0 < f1) { loadv_nt<T, V>(u + f0 * n + g, cu); loadv_nt<T, V>(v + f0 * n + g, cv); }
    for (long long f = f0; f < f1; ++f) {
        if (f + 1 < f1) { loadv_nt<T, V>(u + (f + 1) * n + g, nu); loadv_nt<T, V>(v + (f + 1) * n + g, nv); }
        double ru[V], rv[V];
#pragma unroll
        for (int i = 0; i < V; ++i) {
            T a, b;
            rotate_uv<T>(cu[i], cv[i], c[i], s[i], a, b);
            ru[i] = (double)a; rv[i] = (double)b;
        }
        storev_nt<T, V>(u_out + f * n + g, ru);
        storev_nt<T, V>(v_out + f * n + g, rv);
        if (f + 1 < f1) {
#pragma unroll
            for (int i = 0; i < V; ++i) { cu[i] = nu[i]; cv[i] = nv[i]; }
        }
    }
}

// k_regrid_points on both wind components of a rotated-pole target at once, the rotation behind it: per target the
// corner codes, the two dx and the two reciprocals are formed once and serve both components; a plane costs eight gathers
// (the next plane's are issued before this plane's two streaming stores).  Each component's value is k_regrid_points' - the
// same expressions in the same order, its pole values from k_zonal_mean_rows run on that component - ROUNDED TO T, and the
// pair of T values goes through rotate_uv: the bits of pgw_regrid_points on each component followed by pgw_rotate_pair.
// An oob target gives NaN in both outputs.  TOUT: each rotated component, rounded once to T - what a `--rotate_winds` file of
// step_02 holds - is converted to TOUT; TOUT = T is the kernel as it was.
template <typename T, typename TOUT = T>
__global__ __launch_bounds__(BLOCK) void k_regrid_points_wind(long long nfield, int nlat_s, int nlon_s, long long ntarg, unsigned int gz,
                                                              const T *__restrict__ src_u, const T *__restrict__ src_v, PointTables tb,
                                                              const double *__restrict__ pole_u, const double *__restrict__ pole_v,
                                                              const double *__restrict__ cs, const double *__restrict__ sn,
                                                              TOUT *__restrict__ u_out, TOUT *__restrict__ v_out) {
    const long long g0 = (long long)blockIdx.x * BLOCK + threadIdx.x;
    const bool active = g0 < ntarg;
    const long long g = active ? g0 : ntarg - 1;
    const bool oob = tb.oob[g] != 0;
    const bool live = active && !oob;
    const int jl = tb.lat_lo[g], jh = tb.lat_hi[g], il = tb.lon_lo[g], ih = tb.lon_hi[g];
    const double ldx = tb.lat_dx[g], odx = tb.lon_dx[g];
    const SharedDivisor by_lDx(tb.lat_Dx[g]), by_oDx(tb.lon_Dx[g]);
    const double rc = cs[g], rs = sn[g];
    int c[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int row = k < 2 ? jl : jh;
        int code = row * nlon_s + ((k & 1) ? ih : il);
        if (row < 0) code = -1;
        if (row >= nlat_s) code = -2;
        c[k] = live ? code : 0;
    }
    const long long plane_s = (long long)nlat_s * nlon_s;
    const long long per = (nfield + gz - 1) / gz;
    const long long f0 = (long long)blockIdx.y * per, f1 = f0 + per < nfield ? f0 + per : nfield;
    auto gather = [&](const T *src, long long f, T (&v)[4]) {
        const T *sp = src + f * plane_s;
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] = sp[c[k] >= 0 ? c[k] : 0];
    };
    auto value = [&](const T (&cur)[4], const double *pole, long long f) {
        double v[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] = c[k] >= 0 ? (double)cur[k] : pole[f * 2 + (-1 - c[k])];
        const double ya = by_lDx.divide(v[2] - v[0]) * ldx + v[0];                // lat pass at the lower lon  :859
        const double yb = by_lDx.divide(v[3] - v[1]) * ldx + v[1];                // lat pass at the upper lon
        return (T)(oob ? __builtin_nan("") : by_oDx.divide(yb - ya) * odx + ya);   // lon pass  :892; what pgw_regrid_points stores
    };
    T cu[4], cv[4], nu[4], nv[4];
    if (f0 < f1) { gather(src_u, f0, cu); gather(src_v, f0, cv); }
    for (long long f = f0; f < f1; ++f) {
        if (f + 1 < f1) { gather(src_u, f + 1, nu); gather(src_v, f + 1, nv); }
        T ur, vr;
        rotate_uv<T>((double)value(cu, pole_u, f), (double)value(cv, pole_v, f), rc, rs, ur, vr);
        if (active) {
            __builtin_nontemporal_store((TOUT)ur, u_out + f * ntarg + g0);        // streaming, as k_regrid_points
            __builtin_nontemporal_store((TOUT)vr, v_out + f * ntarg + g0);
        }
        if (f + 1 < f1) {
#pragma unroll
            for (int k = 0; k < 4; ++k) { cu[k] = nu[k]; cv[k] = nv[k]; }
        }
    }
}

// =====================================================================================
// a9  surface riders              step_03_apply_to_era.py:103-146, functions.py:1145-1186
// =====================================================================================
constexpr int MAX_SOIL = 16;
struct SoilTable { double w[MAX_SOIL]; int n; };     // w = exp(-depth/2.8), computed on the host

// ---- rules every rider kernel follows: one statement each ------------------------------------------------------------
// The sea-ice update (step_03:105-107) of one stored fraction `s0` and its delta `d0`.  f32_delta: reference mode and the
// instant IS a record of the delta (no time interpolation: that delta stays the file's float32, functions.py:282-283) -
// numpy then takes `siconc / 100` and the sum onto the ice in float32.  REF: what the blend sees is the float32 value
// stored back into the file's array.
template <typename T, bool REF>
__device__ __forceinline__ double sea_ice_update(double s0, double d0, bool f32_delta) {
    double v = s0 + d0 / 100;                                         // step_03:105
    if (f32_delta) v = (double)((float)s0 + (float)d0 / 100.0f);
    v = fmin(fmax(v, 0.0), 1.0);                                      // :106-107
    if (s0 != s0 || d0 != d0) v = __builtin_nan("");                  // np.clip keeps NaN
    return REF ? (double)(T)v : v;
}

// integrate_tos (functions.py:1173-1184): ts where sea ice or tos is missing, else the land+ice fraction of ts and the rest
// of tos.  REF: `ice + land` and `1 - frac` are float32 operations on the file's float32 fractions (:1183-1184).  f32_ts /
// f32_tos: that delta is a float32 record (see sea_ice_update) - numpy takes every product in the dtype of ITS delta, the
// sum in float32 only if both are.
template <bool REF>
__device__ __forceinline__ double tos_ts_blend(double ice0, double lf, double tos, double ts, bool f32_ts, bool f32_tos) {
    double comb = ts;                                                 // functions.py:1180-1181
    if (ice0 == ice0 && tos == tos) {                                 // :1173
        double fr, omf;
        if (REF) {
            float f = fminf(fmaxf((float)ice0 + (float)lf, 0.0f), 1.0f);
            if ((float)lf != (float)lf) f = __builtin_nanf("");
            fr = (double)f; omf = (double)(1.0f - f);
        } else {
            fr = fmin(fmax(ice0 + lf, 0.0), 1.0);                     // :1183
            if (lf != lf) fr = __builtin_nan("");                     // np.clip keeps NaN
            omf = 1 - fr;
        }
        double p_ts = fr * ts, p_tos = omf * tos;                     // :1184, numpy's promotion operand by operand
        if (f32_ts) p_ts = (double)((float)fr * (float)ts);           // float32 frac * float32 record
        if (f32_tos) p_tos = (double)((float)omf * (float)tos);
        comb = p_ts + p_tos;
        if (f32_ts && f32_tos) comb = (double)((float)p_ts + (float)p_tos);
    }
    return comb;
}

// One point of the riders: the updated sea ice of element i = t * ncol + c and delta_ts_combined (step_03:118-125) there.
// Every delta file has its own time axis, so each DeltaSrc has its own bracket and its own float32-record flag.
template <typename T>
struct RiderSrc { const T *sic; DeltaSrc<T> dsic, dtos, dts; const T *land; };
struct RiderPoint { double ice, comb; };
template <typename T, bool REF>
__device__ __forceinline__ RiderPoint rider_point(const RiderSrc<T> &r, long long i, long long t, long long c) {
    const bool f32_delta = REF && !r.dsic.a, f32_ts = REF && !r.dts.a, f32_tos = REF && !r.dtos.a;
    auto ice_of = [&](long long k) { return sea_ice_update<T, REF>((double)r.sic[k], r.dsic.template get<REF>(k), f32_delta); };
    RiderPoint p;
    p.ice = ice_of(i);
    const double ice0 = (t == 0) ? p.ice : ice_of(c);                 // .isel(time=0), :121-122
    // tos and ts are read before land: the order of the loads decides which product the compiler names first in the blend's
    // commutative sum, and so which NaN a NaN land fraction leaves there (+NaN from frac * ts, -NaN from (1 - frac) * tos).
    // The sign of a NaN is no part of the contract (numpy promises none, the tests compare NaN positions): this order only
    // keeps the bytes the kernels wrote before they shared this text
    const double tos = r.dtos.template get<REF>(i), ts = r.dts.template get<REF>(i);
    p.comb = tos_ts_blend<REF>(ice0, (double)r.land[c], tos, ts, f32_ts, f32_tos);
    return p;
}

// delta_soilt of one layer (step_03:139-142) around `cl`, the annual mean ts delta (:134-136)
__device__ __forceinline__ double soil_delta(const SoilTable &soil, int s, double cl, double comb) {
    return cl + soil.w[s] * (comb - cl);
}

// replace_delta_sfc (functions.py:343-366) on many ascending-pressure columns: source_P is the
// broadcast 1-D table, delta (ntime, S, ncol) ascending order; outputs the modified columns.
// T: the delta (and its output column); TS / TH: delta_sfc and ps_hist; TP: the pressure output.  The surface delta is
// stored in the delta's dtype and ps_hist in the pressures' (np.vectorize allocates its outputs from the first call's
// dtypes: float64 pressures, the delta's own type).
template <typename T, typename TS = T, typename TH = T, typename TP = T, typename PT = PlevTable>
__global__ __launch_bounds__(BLOCK) void k_replace_delta_sfc(PT pt, int ntime, long long ncol,
                                                             const T *__restrict__ delta, const TS *__restrict__ dsfc,
                                                             const TH *__restrict__ pshist, TP *__restrict__ outP,
                                                             T *__restrict__ outD, DevStatus *st) {
    static_assert(kernarg_bytes<PT, int, long long, void *, void *, void *, void *, void *, void *>() <= KERNARG_LIMIT, "kernel arguments");
    __shared__ double s_p[PT::CAP];
    const int S = pt.n;
    stage_plev(pt.p, s_p, BLOCK);
    __syncthreads();
    long long flat = (long long)blockIdx.x * BLOCK + threadIdx.x;
    if (flat >= (long long)ntime * ncol) return;
    long long t = flat / ncol, c = flat - t * ncol;
    long long base = t * S * ncol + c;
    double ps = (double)pshist[flat], ds = (double)dsfc[flat];
    const SfcLevel sl = sfc_level(pt, s_p, ps, st, flat);
    for (int i = 0; i < S; ++i) {
        double P = s_p[i], D = (double)delta[base + (long long)i * ncol];
        if (sl.ksfc >= 0) {
            if (i == sl.ksfc) { P = ps; D = ds; }
            else if (sl.fill && i > sl.ksfc) D = ds;
        }
        outP[base + (long long)i * ncol] = (TP)P;
        outD[base + (long long)i * ncol] = (T)D;
    }
}

// integrate_tos (functions.py:1145-1186), flat over n
template <typename T>
__global__ __launch_bounds__(BLOCK) void k_integrate_tos(long long n, const T *__restrict__ tos, const T *__restrict__ ts,
                                                         const T *__restrict__ land, const T *__restrict__ ice,
                                                         T *__restrict__ out) {
    long long i = (long long)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    out[i] = (T)tos_ts_blend<false>((double)ice[i], (double)land[i], (double)tos[i], (double)ts[i], false, false);
}

// integrate_tos in the reference's dtype flow: every operand in its own storage type, the blend (:1183-1184) in numpy's
// promoted type at every node (C++'s usual arithmetic conversions; np.clip keeps the dtype of its array), written into the
// float64 array of :1180 (np.ones)
template <typename TO_, typename TS, typename TL, typename TI>
__global__ __launch_bounds__(BLOCK) void k_integrate_tos_mixed(long long n, const TO_ *__restrict__ tos, const TS *__restrict__ ts,
                                                               const TL *__restrict__ land, const TI *__restrict__ ice,
                                                               double *__restrict__ out) {
    long long i = (long long)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    const TO_ o = tos[i];
    const TS s = ts[i];
    const TI ic = ice[i];
    double r = (double)s;                                           // :1180-1181
    if (ic == ic && o == o) {                                       // :1173
        auto fr = ic + land[i];
        fr = (fr < 0) ? decltype(fr)(0) : ((fr > 1) ? decltype(fr)(1) : fr);      // :1183: NaN stays NaN
        r = (double)(fr * s + (decltype(fr)(1) - fr) * o);          // :1184
    }
    out[i] = r;
}

// p_ref_inp = None (step_03:219-253 with determine_p_ref, functions.py:583-598): per column the first
// plev (file order) with 0.95*ps_era > p and 0.95*ps_pgw > p, never below the previous pass's choice;
// also applies delta_ps += adj_ps (step_03:192) and gathers g * zg-delta at the chosen level (:292-295).
template <typename T, bool REF>
__global__ __launch_bounds__(BLOCK) void k_local_p_ref(PlevTable pt /* p[] in FILE order here */, double akN, double bkN,
                                                       long long n, const T *__restrict__ PS,
                                                       double *__restrict__ delta_ps, const double *__restrict__ adj_ps,
                                                       DeltaSrc<T> zg /* (nplev, ncol) records */, long long ncol, int first_pass,
                                                       double *__restrict__ p_ref, int *__restrict__ p_idx,
                                                       double *__restrict__ dphi, DevStatus *st) {
    long long i = (long long)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    double dps = next_delta_ps<REF>(delta_ps[i], adj_ps[i]);        // step_03:192
    delta_ps[i] = dps;
    double ps0 = (double)PS[i];
    double p_min_era = (akN + ps0 * bkN) * 0.95;                    // :227-228
    double p_min_pgw = (akN + ps_of<REF>(ps0, dps) * bkN) * 0.95;   // :229-230
    double p = __builtin_nan("");
    int k = -1;
    for (int j = 0; j < pt.n; ++j) {
        if ((p_min_era > pt.p[j]) && (p_min_pgw > pt.p[j])) { p = pt.p[j]; k = j; break; }   // functions.py:593-596
    }
    if (k >= 0 && !first_pass) {
        double last = p_ref[i];
        if (last < p) { p = last; k = p_idx[i]; }                    // min(p, p_ref_last)  :598
    }
    if (k < 0) { report(st, 19, i); p_ref[i] = p; p_idx[i] = -1; dphi[i] = p; return; }   // step_03:245-251
    p_ref[i] = p;
    p_idx[i] = k;
    long long t = i / ncol, c = i - t * ncol;
    dphi[i] = zg.template get<REF>((t * pt.n + k) * ncol + c) * CON_G;            // step_03:292-295
}

// step_03:192-193.  apply_adj = 0: delta_ps already carries this pass's increment (k_local_p_ref applied it), only
// ps_pgw = PS + delta_ps is formed.  REF: the float32 sums of the reference on float32 files (next_delta_ps, ps_of).
template <typename T, bool REF = false>
__global__ __launch_bounds__(BLOCK) void k_update_ps(long long n, const T *__restrict__ PS, double *__restrict__ delta_ps,
                                                     const double *__restrict__ adj_ps, T *__restrict__ ps_out, int apply_adj = 1) {
    long long i = (long long)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    double d = delta_ps[i];
    if (apply_adj) { d = next_delta_ps<REF>(d, adj_ps[i]); delta_ps[i] = d; }
    ps_out[i] = (T)ps_of<REF>((double)PS[i], d);
}

// g * time-interpolated zg delta at p_ref -> fp64 loop constant (step_03:292-295)
// REF: a record that needed no time interpolation stays float32 (functions.py:282-283) and `* CON_G` is a float32 product
template <typename T, bool REF>
__global__ __launch_bounds__(BLOCK) void k_dphi_clim(long long n, DeltaSrc<T> z, double g, double *__restrict__ out,
                                                     double *__restrict__ zero_a, double *__restrict__ zero_b) {
    long long i = (long long)blockIdx.x * BLOCK + threadIdx.x;
    if (i < n) {
        if (REF && !z.a) out[i] = (double)((float)z.b[i] * (float)g);
        else out[i] = z.template get<REF>(i) * g;
        if (zero_a) { zero_a[i] = 0.0; zero_b[i] = 0.0; }          // delta_ps, adj_ps of the loop start (step_03:182-184)
    }
}

// -------------------------------------------------------------------------------------
// Several passes of the loop in ONE launch (fixed p_ref).  A column's trajectory delta_ps(k) depends on that column
// alone - only the stopping test max|err| <= thresh is global (step_03:189, 308) - so a block can run `npass` passes
// on its columns back to back and leave, per pass, the block maxima (status block k) and the delta_ps the pass used
// (dps_hist[k]); the host then applies the reference's control flow to the recorded maxima and finalises from the
// first pass that met the threshold.  Passes beyond it were speculated and are discarded.
// What this buys is NOT memory traffic (the pass is bound by fp64 issue and latency, not by HBM: the float32-storage
// build reads half the bytes in the same time) but the fixed cost of a launch (block dispatch, table staging, tail:
// 0.03-0.045 ms of a 0.22 ms pass) and one host round trip per pass.  Each pass re-reads its rows (L2 / Infinity Cache / HBM).
// `first` != 0 (first launch of a file): phi_ref of the ERA state (step_03:280-287) and g * dzg (:292-295) are computed
// here and stored for continuation launches; delta_ps = adj_ps = 0 (:182-184).
// FLAGGED (with first != 0, npass = 1): the launch that follows a k_delta_quad<.., FUSE = true>.  That kernel has done the
// ERA-state scan and pass 1 for every group of 64 columns whose byte in `flags` is 0; here only the waves that hold a
// flagged column run (scan, zeroed state, pass 1, for all of their columns: the same bits), the others leave at once, and
// thread 0 folds the errors of the delta kernel's ERA-state scan (`st_era`) into `st0`.  The passes after the first then
// run as a continuation launch (first = 0) of the unchanged FLAGGED = false instantiation.
// -------------------------------------------------------------------------------------
constexpr int MULTI_MAX_PASS = 8;
// Storage flows whose loop kernel takes the speculative QV store of PGW_OPT_QV_FROM_PASS (TL = storage type of the PGW level
// arrays, REF = reference-dtype mode); an excluded flow compiles the parent's kernel.  DESIGN.md section 4 has the figures.
// float32 fast mode is excluded: its loop kernel lost more (1.18 -> 1.30 ms) than its finalize kernel, which moves half the
// bytes, gained (0.13 -> 0.06 ms).
template <typename TL, bool REF> constexpr bool QV_FROM_PASS = sizeof(TL) == 8;
// ... and whose storing pass goes on to the first hybrid level and writes ps_pgw (PGW_OPT_FINISH_IN_PASS).  float32 files in
// reference-dtype mode are excluded: their loop launch grew by 0.09 ms (1.33 -> 1.42 ms) for a finalize kernel of 0.12 ms, and
// the per-file figures of the two builds overlapped; they compile the parent's kernel.
template <typename TL, bool REF> constexpr bool FINISH_IN_PASS = QV_FROM_PASS<TL, REF> && !REF;
#ifndef MULTI_MINW
#define MULTI_MINW 4      // 128 VGPRs (12 bytes of scratch per lane): 1.28 -> 1.21 ms against 3 waves / 136 VGPRs; 5 waves spill 132 bytes and lose
#endif
// LOCAL: settings.p_ref_inp = None (step_03:219-253) - the reference level is chosen per column and pass (the first delta
// level, in file order, that lies above 0.95 of the lowest half-level pressure of both states, functions.py:583-598; never
// lower than in the pass before, :598), phi_ref of the ERA state is taken at that level (:280-287: recomputed here only
// when the level changed, it depends on nothing else) and g * dzg at it (:292-295).  `zg` then holds the full
// (nplev, ncol) records, `pt.p` the plev coordinate in file order, `p_ref_col` / `p_idx_col` the per-column memory that a
// continuation launch resumes from.  One column per lane (V = 1).
// The table is zg's plev axis, which is not the axis of ta / hur / ua / va when zg comes from another file (CFday: 99
// levels against Emon / Amon's 19 to 34).  It stays the narrow table: the loop kernel sits on its register budget
// (MULTI_MINW) and a zg file has no more levels than that.
struct LocalPRef { PlevTable pt; double akN, bkN; double *p_ref_col; int *p_idx_col; };
static_assert(kernarg_bytes<LocalPRef, Levels, int, long long, void *, void *, void *, void *, void *, void *, DeltaSrc<double>, void *,
                            void *, void *, void *, void *, double, double, int, int, void *, void *, void *, void *, void *, int,
                            void *, void *>() <= KERNARG_LIMIT, "k_ps_loop_multi: kernel arguments");

template <typename T, typename TL, int V, int U, bool REF, bool LOCAL, bool FLAGGED = false>
__global__ __launch_bounds__(BLOCK, MULTI_MINW) void k_ps_loop_multi(Levels lv, int ntime, long long ncol,
                                                         const T *__restrict__ Tera, const T *__restrict__ QVera,
                                                         const TL *__restrict__ ta, const TL *__restrict__ evap,
                                                         const T *__restrict__ PS, const T *__restrict__ FIS,
                                                         DeltaSrc<T> zg, double *__restrict__ phi_ref_era,
                                                         double *__restrict__ dphi_clim,
                                                         double *__restrict__ delta_ps, double *__restrict__ adj_ps,
                                                         double *__restrict__ dps_hist /* [npass][ntime*ncol] */,
                                                         double p_ref_s, double adj_factor, int first, int npass,
                                                         DevStatus *st0 /* errors of the ERA-state scan */,
                                                         DevStatus *st /* [npass] */, LocalPRef loc,
                                                         const unsigned char *__restrict__ flags = nullptr,
                                                         const DevStatus *st_era = nullptr,
                                                         TL *__restrict__ hus_out = nullptr, int l_start = 0,
                                                         unsigned short *__restrict__ marks = nullptr,
                                                         T *__restrict__ ps_out = nullptr) {
    static_assert(!LOCAL || V == 1, "local p_ref: one column per lane");
    static_assert(!FLAGGED || !LOCAL, "the fused first pass needs a fixed p_ref");
    constexpr bool QVP = QV_FROM_PASS<TL, REF> && !LOCAL && !FLAGGED;
    if constexpr (FLAGGED) {
        // Nothing is staged before the flags are read: after a fused delta kernel almost every block finds none of its waves
        // flagged and leaves here, without the tables and their barrier (all this launch did for 52 us).
        long long gf = (long long)blockIdx.x * BLOCK + threadIdx.x;
        const long long ngf = (long long)ntime * ncol / V;
        if (gf >= ngf) gf = ngf - 1;
        bool flagged = false;
#pragma unroll
        for (int v = 0; v < V; ++v) flagged = flagged || flags[(gf * V + v) >> 6] != 0;
        if (blockIdx.x == 0 && threadIdx.x == 0 && st_era->code != 0) report(st0, st_era->code, (long long)st_era->col);
        if (!__syncthreads_or(flagged)) return;
    }
    __shared__ unsigned long long s_max[MULTI_MAX_PASS];          // per pass: max |err| as ordered bits, #valid, levels read
    __shared__ unsigned int s_valid[MULTI_MAX_PASS];
    __shared__ unsigned long long s_touched[MULTI_MAX_PASS];
    __shared__ double s_lev[LEVTAB_DOUBLES];
    __shared__ unsigned long long s_stored;                       // QVP: level-columns of QV this block's last pass stored
    if (threadIdx.x < MULTI_MAX_PASS) { s_max[threadIdx.x] = 0ull; s_valid[threadIdx.x] = 0u; s_touched[threadIdx.x] = 0ull; }
    if constexpr (QVP) { if (threadIdx.x == 0) s_stored = 0ull; }
    LevTab lt = stage_levels<true, true>(lv, s_lev, BLOCK);        // ends with a barrier
    const long long n2 = (long long)ntime * ncol;
    long long g = (long long)blockIdx.x * BLOCK + threadIdx.x;
    long long ngroups = n2 / V;
    // The per-pass wave reductions below (wave_max, the __shfl_xor sum) need all 64 lanes: a lane beyond the last group
    // (1440 x 721 columns leave 32 lanes of the last wave idle) walks the last group again - no stores, nothing contributed -
    // instead of sitting out in a divergent branch, where the shuffles would read its registers undefined (a zero from
    // there made an all-NaN partial wave "valid" with |err| = 0).
    const bool live = g < ngroups;
    if (!live) g = ngroups - 1;
    bool run = true;
    if (FLAGGED) {
        const long long c2 = g * V;
        bool flagged = false;
#pragma unroll
        for (int v = 0; v < V; ++v) flagged = flagged || flags[(c2 + v) >> 6] != 0;
        run = __any(flagged);
    }
    if (run) {
        ColIdx ix = col_index(g, V, ncol);
        const int N = lv.nlev;
        long long c2 = ix.t * ncol + ix.c;
        const long long lbase = ix.t * N * ncol + ix.c;
        double ps0[V], z[V], dps[V], adj[V], pref[V], tlow[V], phi_ref[V], phi_era[V], dphi[V];
        int idx = -2;                                              // LOCAL: index of the column's current level (-2: none yet)
        loadv<T, V>(PS + c2, ps0);
        loadv<T, V>(FIS + c2, z);
#pragma unroll
        for (int v = 0; v < V; ++v) pref[v] = p_ref_s;
        if (first) {
            if (!LOCAL) {
                int touched0 = 0;
                scan_columns<T, V, U, true, REF>(lv, lt, ncol, Tera + lbase, QVera + lbase, ps0, z, pref, 0, st0, c2, phi_era, tlow, touched0);
#pragma unroll
                for (int v = 0; v < V; ++v) {
                    if (REF && !zg.a) dphi[v] = (double)((float)zg.b[c2 + v] * (float)CON_G);      // see k_dphi_clim
                    else dphi[v] = zg.template get<REF>(c2 + v) * CON_G;                             // step_03:292-295
                }
                if (live) {
                    storev<double, V>(phi_ref_era + c2, phi_era);
                    storev<double, V>(dphi_clim + c2, dphi);
                }
            }
#pragma unroll
            for (int v = 0; v < V; ++v) { dps[v] = 0.0; adj[v] = 0.0; }                              // :182-184
        } else {
            loadv<double, V>(phi_ref_era + c2, phi_era);
            loadv<double, V>(dphi_clim + c2, dphi);
            loadv<double, V>(delta_ps + c2, dps);
            loadv<double, V>(adj_ps + c2, adj);
            if (LOCAL) { pref[0] = loc.p_ref_col[c2]; idx = loc.p_idx_col[c2]; }
        }
        int low = N;                                               // QVP: lowest level index the last pass processed
        for (int k = 0; k < npass; ++k) {
            double ps[V];
#pragma unroll
            for (int v = 0; v < V; ++v) {
                dps[v] = next_delta_ps<REF>(dps[v], adj[v]);              // step_03:192
                ps[v] = ps_of<REF>(ps0[v], dps[v]);                       // :193
            }
            if (live) storev<double, V>(dps_hist + (long long)k * n2 + c2, dps);
            if (LOCAL) {
                const double p_min_era = (loc.akN + ps0[0] * loc.bkN) * 0.95;                  // :227-228
                const double p_min_pgw = (loc.akN + ps[0] * loc.bkN) * 0.95;                   // :229-230
                double p = __builtin_nan("");
                int j = -1;
                for (int i = 0; i < loc.pt.n; ++i)
                    if ((p_min_era > loc.pt.p[i]) && (p_min_pgw > loc.pt.p[i])) { p = loc.pt.p[i]; j = i; break; }   // functions.py:593-596
                if (j >= 0 && idx >= 0 && pref[0] < p) { p = pref[0]; j = idx; }               // min(p, p_ref_last)  :598
                if (j < 0) { report(st + k, 19, c2); p = __builtin_nan(""); }                   // step_03:245-251
                if (j != idx) {                                                                 // (first pass: idx == -2)
                    pref[0] = p;
                    idx = j;
                    if (j >= 0) {
                        int touched0 = 0;
                        scan_columns<T, V, U, true, REF>(lv, lt, ncol, Tera + lbase, QVera + lbase, ps0, z, pref, 0, st + k, c2, phi_era,
                                                         tlow, touched0);                       // :280-287
                        dphi[0] = zg.template get<REF>((ix.t * loc.pt.n + j) * ncol + ix.c) * CON_G;          // :292-295
                    } else {
                        phi_era[0] = p; dphi[0] = p;
                    }
                }
            }
            int touched = 0;
            if constexpr (QVP) {
                // the last pass of the launch also stores its q into hus_pgw (see above), in an instantiation of its own: the
                // other passes keep the parent's loop.  (One body with l_lim = N for them measured the same per file, 3.2345
                // vs 3.2355 ms, but needs 28 bytes of scratch against 20: DESIGN.md section 4.)
                const bool last = k == npass - 1 && hus_out;
                const long long qdiff = (const char *)hus_out - (const char *)evap;
                if (last) scan_columns<TL, V, U, false, REF, 2>(lv, lt, ncol, ta + lbase, evap + lbase, ps, z, pref, 0, st + k, c2,
                                                                phi_ref, tlow, touched, qdiff, l_start, live, &low);
                else scan_columns<TL, V, U, false, REF, 1>(lv, lt, ncol, ta + lbase, evap + lbase, ps, z, pref, 0, st + k, c2, phi_ref,
                                                           tlow, touched);
            } else
                scan_columns<TL, V, U, false, REF>(lv, lt, ncol, ta + lbase, evap + lbase, ps, z, pref, 0, st + k, c2, phi_ref, tlow,
                                                   touched);
            double amax = -1.0;
#pragma unroll
            for (int v = 0; v < V; ++v) {
                double err = (phi_ref[v] - phi_era[v]) - dphi[v];                         // :289,298
                const double fps = REF ? (double)((float)(-adj_factor) * (float)ps[v]) : -adj_factor * ps[v];
                adj[v] = fps / (CON_RD * tlow[v]) * err;                                  // :301-304
                double ae = fabs(err);
                if (ae == ae) amax = fmax(amax, ae);                                      // :308 skipna
            }
            if (!live) { amax = -1.0; touched = 0; }
            double wm = wave_max(amax);
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) touched += __shfl_xor(touched, off, 64);
            if ((threadIdx.x & 63) == 0) {
                if (wm >= 0.0) { atomicMax(&s_max[k], dbits(wm)); atomicAdd(&s_valid[k], 1u); }
                atomicAdd(&s_touched[k], (unsigned long long)touched);
            }
        }
        if (live) {
            storev<double, V>(delta_ps + c2, dps);        // state after the last pass: a continuation launch resumes here
            storev<double, V>(adj_ps + c2, adj);
        }
        if constexpr (QVP) {
            if (hus_out) {
                // PGW_OPT_FINISH_IN_PASS (ps_out given): the wave goes on from where its scan stopped to l_start, with the
                // quotient of the storing pass and no geopotential, and writes ps_pgw of this pass - what k_finalize_ps_hus
                // would do for these columns from this pass's delta_ps.  A loop of its own, here where the scan's and the
                // pass's registers are dead, with the next XU rows of e in flight; e is read for the last time if this pass
                // is the converged one.  Nothing to do for a wave that walked to the top (ps < ps_mono_min, NaN ps).
                if constexpr (FINISH_IN_PASS<TL, REF>) if (ps_out) {
                    constexpr int XU = 4;
                    double ps[V], en[XU][V];
#pragma unroll
                    for (int v = 0; v < V; ++v) ps[v] = ps_of<REF>(ps0[v], dps[v]);
                    const TL *pe = evap + lbase;
                    const long long qdiff = (const char *)hus_out - (const char *)evap;
                    const int top = __builtin_amdgcn_readfirstlane(low) - 1;         // (the stop is wave-uniform)
#pragma unroll
                    for (int u = 0; u < XU; ++u) {
                        const int lu = (top - u) > l_start ? (top - u) : l_start;
                        if (top >= l_start) loadv_nt<TL, V>(pe + (long long)lu * ncol, en[u]);
                    }
                    for (int l = top; l >= l_start; l -= XU) {
                        double e[XU][V];
#pragma unroll
                        for (int u = 0; u < XU; ++u)
#pragma unroll
                            for (int v = 0; v < V; ++v) e[u][v] = en[u][v];
                        if (l - XU >= l_start) {
#pragma unroll
                            for (int u = 0; u < XU; ++u) {
                                const int lu = (l - XU - u) > l_start ? (l - XU - u) : l_start;
                                loadv_nt<TL, V>(pe + (long long)lu * ncol, en[u]);
                            }
                        }
#pragma unroll
                        for (int u = 0; u < XU; ++u) {
                            const int lc = l - u;
                            if (lc >= l_start) {
                                const double am = lt.akm[lc], bm = lt.bkm[lc];
                                double qs[V];
#pragma unroll
                                for (int v = 0; v < V; ++v) {
                                    const double pm = am + ps[v] * bm;
                                    qs[v] = SharedDivisor(pm - (1 - CON_MW_MD) * e[u][v]).divide(CON_MW_MD * e[u][v]);
                                }
                                // the row of hus_pgw as the lane's `pe` plus one uniform byte offset, as in scan_columns
                                const long long ob = (long long)lc * ncol * (long long)sizeof(TL) + qdiff;
                                const unsigned int olo = __builtin_amdgcn_readfirstlane((unsigned int)ob);
                                const unsigned int ohi = __builtin_amdgcn_readfirstlane((unsigned int)((unsigned long long)ob >> 32));
                                const long long ou = (long long)(((unsigned long long)ohi << 32) | olo);
                                if (live) storev_nt<TL, V>((TL *)((char *)const_cast<TL *>(pe) + ou), qs);
                            }
                        }
                    }
                    if (live) storev<T, V>(ps_out + c2, ps);
                    if (low > l_start) low = l_start;
                }
                // the levels low .. N-1 (from l_start on) of these columns now hold the q of pass npass-1; the stop is
                // wave-uniform, so one lane speaks for the wave's live columns
                if (live) {
#pragma unroll
                    for (int v = 0; v < V; ++v) marks[c2 + v] = (unsigned short)low;
                }
                const int stored = N - (low > l_start ? low : l_start);
                const unsigned long long nlive = __popcll(__ballot(live));
                if ((threadIdx.x & 63) == 0 && stored > 0) atomicAdd(&s_stored, nlive * V * (unsigned long long)stored);
            }
        }
        if (LOCAL && live) {
            loc.p_ref_col[c2] = pref[0]; loc.p_idx_col[c2] = idx;
            phi_ref_era[c2] = phi_era[0]; dphi_clim[c2] = dphi[0];
        }
    }
    __syncthreads();
    if ((int)threadIdx.x < npass) {
        const int k = threadIdx.x;
        if (s_valid[k]) {
            atomicMax(&st[k].max_bits, s_max[k]);
            atomicAdd(&st[k].valid, 1ull);
        }
        atomicAdd(&st[k].levels_touched, s_touched[k]);
    }
    if constexpr (QVP) {
        if (threadIdx.x == 0 && hus_out && s_stored) atomicAdd(&st[npass - 1].qv_stored, s_stored);
    }
}

// surface riders with the time lerp of the three 2-D deltas fused in (step_03:103-146): rider_point and the sums onto the
// ERA fields, in the storage type.  Every output is optional (pgw_surface_update; pgw_step03_file writes all but comb_out).
template <typename T, bool REF>
__global__ __launch_bounds__(BLOCK) void k_surface_update_lerp(int ntime, long long ncol, SoilTable soil, RiderSrc<T> r,
                                                               const T *__restrict__ clim, const T *__restrict__ tskin,
                                                               const T *__restrict__ tso, T *__restrict__ sic_out,
                                                               T *__restrict__ comb_out, T *__restrict__ tskin_out,
                                                               T *__restrict__ tso_out) {
    long long i = (long long)blockIdx.x * BLOCK + threadIdx.x;
    long long n = (long long)ntime * ncol;
    if (i >= n) return;
    long long t = i / ncol, c = i - t * ncol;
    const RiderPoint p = rider_point<T, REF>(r, i, t, c);
    if (sic_out) sic_out[i] = (T)p.ice;
    if (comb_out) comb_out[i] = (T)p.comb;
    if (tskin_out) tskin_out[i] = (T)((double)tskin[i] + p.comb);     // step_03:124
    if (tso_out) {
        double cl = (double)clim[c];                                  // annual mean ts delta :134-136
#pragma unroll
        for (int s = 0; s < MAX_SOIL; ++s) {
            if (s < soil.n) {
                long long o = (t * soil.n + s) * ncol + c;
                tso_out[o] = (T)((double)tso[o] + soil_delta(soil, s, cl, p.comb));   // :139-144
            }
        }
    }
}

// The two surface deltas themselves (step_03 --debug_mode interpolate_full): delta_ts_combined (step_03:118-125) and
// delta_soilt (:139-143) as the float64 arrays the reference holds (np.ones in integrate_tos, functions.py:1180; float64
// exp(-soil1 / 2.8)): rider_point and soil_delta as k_surface_update_lerp calls them, without the sums onto the ERA fields
// and the rounding to the storage type.
template <typename T, bool REF>
__global__ __launch_bounds__(BLOCK) void k_surface_deltas(int ntime, long long ncol, SoilTable soil, RiderSrc<T> r,
                                                          const T *__restrict__ clim, double *__restrict__ comb_out,
                                                          double *__restrict__ dsoil_out) {
    long long i = (long long)blockIdx.x * BLOCK + threadIdx.x;
    long long n = (long long)ntime * ncol;
    if (i >= n) return;
    long long t = i / ncol, c = i - t * ncol;
    const double comb = rider_point<T, REF>(r, i, t, c).comb;
    comb_out[i] = comb;                                               // step_03:125
    if (dsoil_out) {
        double cl = (double)clim[c];                                  // annual mean ts delta :134-136
#pragma unroll
        for (int s = 0; s < MAX_SOIL; ++s) {
            if (s < soil.n) dsoil_out[(t * soil.n + s) * ncol + c] = soil_delta(soil, s, cl, comb);   // :139-142
        }
    }
}

// =====================================================================================
// step_02 `smoothing`: filter_data / harmonic_ac_analysis          functions.py:603-740
// in / out (ntime, inner): one thread per column (level, y, x flattened), lanes along x, so each time step of a
// wave is one coalesced row segment.  Pass 1 streams the series once (NaN test, sum, three cos / sin projections),
// pass 2 writes mean + the three harmonics.  cos / sin tables [3][ntime] come from the host (numpy, evaluated as
// the reference does at :716, 727) and are staged in LDS; every lane reads the same entry (broadcast).
// =====================================================================================
template <typename T, int U>
__global__ __launch_bounds__(BLOCK) void k_harmonic_smooth(int ntime, long long inner, const double *__restrict__ tabs,
                                                           const T *__restrict__ in, T *__restrict__ out) {
    extern __shared__ double s_tab[];                 // cos[3][ntime], sin[3][ntime]
    for (int i = threadIdx.x; i < 6 * ntime; i += BLOCK) s_tab[i] = tabs[i];
    __syncthreads();
    const long long c = (long long)blockIdx.x * BLOCK + threadIdx.x;
    if (c >= inner) return;
    const double *c1 = s_tab, *c2 = s_tab + ntime, *c3 = s_tab + 2 * ntime;
    const double *s1 = s_tab + 3 * ntime, *s2 = s_tab + 4 * ntime, *s3 = s_tab + 5 * ntime;
    const T *pi = in + c;
    double sum = 0, a1 = 0, a2 = 0, a3 = 0, b1 = 0, b2 = 0, b3 = 0;
    bool nan = false;
    for (int t0 = 0; t0 < ntime; t0 += U) {
        double x[U];
#pragma unroll
        for (int u = 0; u < U; ++u) x[u] = (double)SIG_LD(pi + (long long)(t0 + u < ntime ? t0 + u : ntime - 1) * inner);
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int t = t0 + u;
            if (t < ntime) {
                nan |= (x[u] != x[u]);                                   // :694
                sum += x[u];                                             // :699
                a1 += x[u] * c1[t]; b1 += x[u] * s1[t];                  // :728-730
                a2 += x[u] * c2[t]; b2 += x[u] * s2[t];
                a3 += x[u] * c3[t]; b3 += x[u] * s3[t];
            }
        }
    }
    const double lt = (double)ntime;
    const double mean = sum / lt, f = 2. / lt;
    a1 = f * a1; b1 = f * b1; a2 = f * a2; b2 = f * b2; a3 = f * a3; b3 = f * b3;
    T *po = out + c;
    for (int t = 0; t < ntime; ++t) {
        double h1 = a1 * c1[t] + b1 * s1[t];                             // :733
        double h2 = a2 * c2[t] + b2 * s2[t];
        double h3 = a3 * c3[t] + b3 * s3[t];
        double r = ((h1 + h2) + h3) + mean;                              // :739
        SIG_ST((T)(nan ? __builtin_nan("") : r), po + (long long)t * inner);     // :695-696
    }
}

// =====================================================================================
// step_02 NaN-ignoring interpolation of ocean-grid deltas (tos, siconc)      functions.py:900-1060
// The reference hands two point clouds in planar "metre" coordinates (functions.py:958-1023; host: geodesy.py) to
// pyvista's PolyData.interpolate(points, null_value=nan, radius=R, sharpness=s) (:1038-1048) = VTK's vtkPointInterpolator
// with a vtkGaussianKernel on a RADIUS footprint.  Per target point x (VTK 9.2 vtkGaussianKernel::ComputeWeights,
// vtkPointInterpolator):
//     neighbours  = source points with |x - p|^2 <= R^2 ;  none -> null value (NaN)
//     |x - p|^2 < 256 eps for some p  ->  the value of (the first such) p
//     else  sum_i w_i v_i / sum_i w_i ,  w_i = exp(-(s/R)^2 |x - p_i|^2)
// (VTK divides the weights by their sum first and then forms sum (w_i / W) v_i; here the quotient of the two sums is
// taken once - equal up to rounding; parity with VTK is unpinned anyway: VTK / pyvista / pyproj are not installable.)
// Source points are binned on the host into square cells of edge R (sorted by cell, `cell_start` = first point of each
// cell), so a target looks at its 3 x 3 block of cells.  One thread per target point; all `nm` months of a variable in
// ONE pass (the geometry - the expensive part, one exp per pair - is shared; the reference repeats it 12 times).  A
// month's NaN values are skipped for that month (the reference removes them from that month's cloud, :944-948).
// =====================================================================================
constexpr int GAUSS_MAX_FIELDS = 16;
// One target per thread; the SOURCE points are staged through LDS by the block: the targets of a block (consecutive
// indices: neighbours on the ERA5 grid) need the 3 x 3 cell neighbourhoods of a small box of cells, and for one cell row ix the
// cells iy_lo .. iy_hi are one contiguous run of the cell-sorted source arrays.  The block copies that run in chunks of
// GAUSS_CHUNK points (coordinates and the values of all months: coalesced) into LDS and every thread walks the chunk with
// broadcast reads; a point outside a thread's own neighbourhood fails the radius test (cells are at least one radius wide).
// Per thread the accepted points arrive in the order (ix, iy, p) of a direct walk over its 3 x 3 cells, so the sums are the
// bits of that walk.  The first form of this kernel did walk the cells per thread from global memory: one exposed memory
// latency per source point, 115 ms for 12 months of tos on the 0.25 deg grid at 1.4 waves per SIMD.
// A target with NaN coordinates is inactive.  The host hands the targets over in tiles of 16 x 16 grid points (edge tiles
// filled with such targets): a block's box of cells stays small, and so does the set of points a wave accepts for some of
// its lanes only (a wave runs the weight arithmetic of a point when ANY lane has it within the radius).
constexpr int GAUSS_CHUNK = 256;
// The source walk of one block, shared by k_gauss_interp and k_gauss_points: (cx, cy) is the thread's own cell (used when
// `active`), the block's box of cells is formed from the active threads' cells, and sw / swv / hit / has_hit come back as the
// thread's sums.  Called by every thread of the block (it synchronises).
template <int NM>
__device__ __forceinline__ void gauss_walk(bool active, double x, double y, int cx, int cy, int ncx, int ncy,
                                           const int *__restrict__ cell_start, const double *__restrict__ sx,
                                           const double *__restrict__ sy, const double *__restrict__ sval /* [nsrc][nm] */, int nm,
                                           double r2, double f2, double (&sw)[NM], double (&swv)[NM], double (&hit)[NM],
                                           bool (&has_hit)[NM]) {
    __shared__ double s_x[GAUSS_CHUNK], s_y[GAUSS_CHUNK];
    __shared__ double s_v[GAUSS_CHUNK * NM];
    __shared__ int s_box[4];                                    // cx_min, cx_max, cy_min, cy_max of the block's active targets
    __shared__ int s_nan[GAUSS_CHUNK];                          // the point has a NaN month (rare: the common path tests nothing)
    if (threadIdx.x == 0) { s_box[0] = 0x7fffffff; s_box[1] = -0x7fffffff; s_box[2] = 0x7fffffff; s_box[3] = -0x7fffffff; }
    __syncthreads();
    if (active) { atomicMin(&s_box[0], cx); atomicMax(&s_box[1], cx); atomicMin(&s_box[2], cy); atomicMax(&s_box[3], cy); }
    __syncthreads();
#pragma unroll
    for (int m = 0; m < NM; ++m) { sw[m] = 0.0; swv[m] = 0.0; hit[m] = 0.0; has_hit[m] = false; }
    const double tol = 256.0 * 2.220446049250313e-16;           // vtkMathUtilities::FuzzyCompare(d2, 0.0, eps * 256)
    if (s_box[1] >= s_box[0]) {                                  // at least one active target (uniform over the block)
        int ix_lo = s_box[0] - 1, ix_hi = s_box[1] + 1, iy_lo = s_box[2] - 1, iy_hi = s_box[3] + 1;
        if (ix_lo < 0) ix_lo = 0;
        if (iy_lo < 0) iy_lo = 0;
        if (ix_hi > ncx - 1) ix_hi = ncx - 1;
        if (iy_hi > ncy - 1) iy_hi = ncy - 1;
        for (int ix = ix_lo; ix <= ix_hi && iy_lo <= iy_hi; ++ix) {
            const int p_lo = cell_start[ix * ncy + iy_lo], p_hi = cell_start[ix * ncy + iy_hi + 1];
            for (int p0 = p_lo; p0 < p_hi; p0 += GAUSS_CHUNK) {
                const int cnt = (p_hi - p0 < GAUSS_CHUNK) ? (p_hi - p0) : GAUSS_CHUNK;
                __syncthreads();                                 // the previous chunk has been read by everyone
                for (int q = threadIdx.x; q < cnt; q += BLOCK) { s_x[q] = sx[p0 + q]; s_y[q] = sy[p0 + q]; s_nan[q] = 0; }
                __syncthreads();
                for (int q = threadIdx.x; q < cnt * nm; q += BLOCK) {
                    const int pt = q / nm, m = q - pt * nm;
                    const double v = sval[(long long)p0 * nm + q];
                    s_v[pt * NM + m] = v;
                    if (v != v) s_nan[pt] = 1;
                }
                __syncthreads();
                if (active) {
                    for (int q = 0; q < cnt; ++q) {
                        const double dx = x - s_x[q], dy = y - s_y[q];
                        const double d2 = dx * dx + dy * dy;     // the third coordinate is 0 on both sides (:986-988, 1028-1030)
                        if (!(d2 <= r2)) continue;               // vtkStaticPointLocator::FindPointsWithinRadius
                        const double w = pgw_exp(-f2 * d2);
                        const bool exact = d2 < tol;
                        if (!s_nan[q] && !exact) {               // every month valid, not a coincident point: nothing to test
#pragma unroll
                            for (int m = 0; m < NM; ++m) {
                                if (m < nm) { const double vm = s_v[q * NM + m]; sw[m] += w; swv[m] += w * vm; }
                            }
                            continue;
                        }
#pragma unroll
                        for (int m = 0; m < NM; ++m) {
                            if (m < nm) {
                                const double vm = s_v[q * NM + m];
                                if (vm == vm) {                  // a NaN month of this point: skipped
                                    sw[m] += w; swv[m] += w * vm;
                                    if (exact && !has_hit[m]) { has_hit[m] = true; hit[m] = vm; }
                                }
                            }
                        }
                    }
                }
            }
        }
    }
}

// null_value (:1041) where nothing was in reach, the coincident point's value, else the quotient of the two sums
template <int NM>
__device__ __forceinline__ void gauss_store(long long ntarg, long long i, int nm, const double (&sw)[NM], const double (&swv)[NM],
                                            const double (&hit)[NM], const bool (&has_hit)[NM], double *__restrict__ out) {
#pragma unroll
    for (int m = 0; m < NM; ++m) {
        if (m < nm) {
            double r = __builtin_nan("");
            if (has_hit[m]) r = hit[m];
            else if (sw[m] > 0.0) r = swv[m] / sw[m];
            out[(long long)m * ntarg + i] = r;
        }
    }
}

template <int NM>
__global__ __launch_bounds__(BLOCK) void k_gauss_interp(long long ntarg, const double *__restrict__ tx, const double *__restrict__ ty,
                                                        int ncx, int ncy, double x0, double y0, double inv_h,
                                                        const int *__restrict__ cell_start, const double *__restrict__ sx,
                                                        const double *__restrict__ sy, const double *__restrict__ sval /* [nsrc][nm] */,
                                                        int nm, double r2, double f2, double *__restrict__ out /* [nm][ntarg] */) {
    const long long i = (long long)blockIdx.x * BLOCK + threadIdx.x;
    double x = __builtin_nan(""), y = __builtin_nan("");
    if (i < ntarg) { x = tx[i]; y = ty[i]; }
    const bool active = (x == x) && (y == y);
    int cx = 0, cy = 0;
    if (active) { cx = (int)floor((x - x0) * inv_h); cy = (int)floor((y - y0) * inv_h); }
    double sw[NM], swv[NM], hit[NM];
    bool has_hit[NM];
    gauss_walk<NM>(active, x, y, cx, cy, ncx, ncy, cell_start, sx, sy, sval, nm, r2, f2, sw, swv, hit, has_hit);
    if (i < ntarg) gauss_store<NM>(ntarg, i, nm, sw, swv, hit, has_hit, out);
}

// -------------------------------------------------------------------------------------
// The same interpolation for targets in ANY order (point-wise targets: 2-D lat / lon of a rotated-pole file, a cell list).
// The targets are put into the order of the source's cells on the device, so that a block of 256 consecutive sorted
// positions has a small box of cells to stage, and every result is written to the target's own index:
//   k_gauss_keys     key of the target's cell + histogram of the keys.  The cell index is the walk's floor((x - x0) * inv_h),
//                    clamped in double to [-1, ncx] x [-1, ncy] before the conversion: a target outside the grid can still be
//                    within one radius of a border cell's points; one far away (1e18) lands in the same ring of outside
//                    cells, stages the border cells and accepts nothing.  Cell rows alternate their direction (a snake), so
//                    that the block that runs from the end of one row into the next has neighbouring cells, not a box as
//                    long as the row.  Inside a cell the key goes on with the target's place in GAUSS_SUB x GAUSS_SUB parts of
//                    the cell: a wave runs the weight arithmetic of a point when ANY of its lanes has it within the radius,
//                    so the 64 targets of a wave should lie close together, not anywhere in a cell one radius wide.
//                    Inactive targets (NaN coordinate) get the key behind all cells.
//   k_gauss_scan     exclusive scan of the histogram by one block; n_active = start of the last key.
//   k_gauss_scatter  order[atomicAdd(&start[key], 1)] = i.  The order inside one cell is whatever the atomics give: per thread
//                    the accepted points arrive in the order (ix, iy, p) whatever the block stages, so a target's sums do not
//                    depend on its position.
//   k_gauss_points   the walk on i = order[pos]; positions from n_active on write NaN and walk nothing.
// -------------------------------------------------------------------------------------
__device__ __forceinline__ int gauss_cell(double v, double v0, double inv_h, int nc) {
    double c = floor((v - v0) * inv_h);
    c = c < -1.0 ? -1.0 : c;
    c = c > (double)nc ? (double)nc : c;
    return (int)c;
}

// which of the GAUSS_SUB parts of its cell (index c, not clamped) along one axis the coordinate lies in
constexpr int GAUSS_SUB = 4;
__device__ __forceinline__ int gauss_sub(double v, double v0, double inv_h, int c) {
    double f = ((v - v0) * inv_h - (double)c) * GAUSS_SUB;
    f = f > 0.0 ? f : 0.0;                                       // (a clamped cell: the coordinate lies outside it)
    f = f < (double)(GAUSS_SUB - 1) ? f : (double)(GAUSS_SUB - 1);
    return (int)f;
}

__global__ __launch_bounds__(BLOCK) void k_gauss_keys(int ntarg, const double *__restrict__ tx, const double *__restrict__ ty, int ncx,
                                                      int ncy, double x0, double y0, double inv_h, int *__restrict__ key,
                                                      int *__restrict__ count /* [(ncx + 2) * (ncy + 2) * GAUSS_SUB^2 + 1], zero */) {
    const long long i = (long long)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= ntarg) return;
    const double x = tx[i], y = ty[i];
    int k = (ncx + 2) * (ncy + 2) * (GAUSS_SUB * GAUSS_SUB);
    if (x == x && y == y) {
        const int cx = gauss_cell(x, x0, inv_h, ncx), cy = gauss_cell(y, y0, inv_h, ncy);
        const int row = cx + 1, col = (row & 1) ? ncy - cy : cy + 1;
        k = (row * (ncy + 2) + col) * (GAUSS_SUB * GAUSS_SUB) + gauss_sub(x, x0, inv_h, cx) * GAUSS_SUB + gauss_sub(y, y0, inv_h, cy);
    }
    key[i] = k;
    atomicAdd(&count[k], 1);
}

constexpr int SCAN_BLOCK = 1024;
__global__ __launch_bounds__(SCAN_BLOCK) void k_gauss_scan(int nkey, int *__restrict__ count /* in: counts, out: starts */,
                                                           int *__restrict__ n_active) {
    __shared__ int s_sum[SCAN_BLOCK];
    const int per = (nkey + SCAN_BLOCK - 1) / SCAN_BLOCK;
    const int lo = threadIdx.x * per < nkey ? threadIdx.x * per : nkey;
    const int hi = lo + per < nkey ? lo + per : nkey;
    int sum = 0;
    for (int k = lo; k < hi; ++k) sum += count[k];
    s_sum[threadIdx.x] = sum;
    __syncthreads();
    for (int d = 1; d < SCAN_BLOCK; d <<= 1) {                   // inclusive scan of the per-thread sums
        const int v = threadIdx.x >= d ? s_sum[threadIdx.x - d] : 0;
        __syncthreads();
        s_sum[threadIdx.x] += v;
        __syncthreads();
    }
    int run = s_sum[threadIdx.x] - sum;
    for (int k = lo; k < hi; ++k) {
        const int c = count[k];
        count[k] = run;
        if (k == nkey - 1) *n_active = run;                      // the last key is the inactive targets'
        run += c;
    }
}

__global__ __launch_bounds__(BLOCK) void k_gauss_scatter(int ntarg, const int *__restrict__ key, int *__restrict__ start,
                                                         int *__restrict__ order) {
    const long long i = (long long)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= ntarg) return;
    order[atomicAdd(&start[key[i]], 1)] = (int)i;
}

template <int NM>
__global__ __launch_bounds__(BLOCK) void k_gauss_points(int ntarg, const int *__restrict__ order, const int *__restrict__ n_active,
                                                        const double *__restrict__ tx, const double *__restrict__ ty,
                                                        int ncx, int ncy, double x0, double y0, double inv_h,
                                                        const int *__restrict__ cell_start, const double *__restrict__ sx,
                                                        const double *__restrict__ sy, const double *__restrict__ sval /* [nsrc][nm] */,
                                                        int nm, double r2, double f2, double *__restrict__ out /* [nm][ntarg] */) {
    const long long pos = (long long)blockIdx.x * BLOCK + threadIdx.x;
    const int na = *n_active;
    const int i = pos < ntarg ? order[pos] : -1;
    if ((long long)blockIdx.x * BLOCK >= na) {                             // a block of inactive targets only (uniform over the block)
        if (i >= 0) {
#pragma unroll
            for (int m = 0; m < NM; ++m) if (m < nm) out[(long long)m * ntarg + i] = __builtin_nan("");
        }
        return;
    }
    const bool active = pos < na;
    double x = __builtin_nan(""), y = __builtin_nan("");
    int cx = 0, cy = 0;
    if (active) {
        x = tx[i]; y = ty[i];
        cx = gauss_cell(x, x0, inv_h, ncx); cy = gauss_cell(y, y0, inv_h, ncy);
    }
    double sw[NM], swv[NM], hit[NM];
    bool has_hit[NM];
    gauss_walk<NM>(active, x, y, cx, cy, ncx, ncy, cell_start, sx, sy, sval, nm, r2, f2, sw, swv, hit, has_hit);
    if (i >= 0) gauss_store<NM>(ntarg, i, nm, sw, swv, hit, has_hit, out);
}

// float64 -> float32 (round to nearest even, the conversion numpy's astype does), two elements per lane, optionally byte-reversed
// -------------------------------------------------------------------------------------
// Planar "metre" coordinates of the ocean-grid interpolation (functions.py:958-975, 1010-1023: three pyproj Geod.inv
// calls per point) on the GPU: the arithmetic of pgw4era5_amd/geodesy.py (Vincenty's series arranged so that nothing
// iterates to failure - meridian arc and over-the-pole length from the direct series with azimuth 0, the geodesic between
// two points of one parallel by bisection on the departure azimuth), one point per thread.  Same formulas and iteration
// count as the host form; sin / cos / atan2 are the device library's, so results agree to the last bits (~1e-9 m), not
// bit for bit.
// -------------------------------------------------------------------------------------
namespace geo {
constexpr double A = 6378137.0, F = 1.0 / 298.257223563, B = A * (1.0 - F), PI = 3.14159265358979323846;
struct Series { double a, b, c; };
__device__ __forceinline__ Series series(double cos2_alpha) {
    const double u2 = cos2_alpha * (A * A - B * B) / (B * B);
    Series s;
    s.a = 1 + u2 / 16384 * (4096 + u2 * (-768 + u2 * (320 - 175 * u2)));
    s.b = u2 / 1024 * (256 + u2 * (-128 + u2 * (74 - 47 * u2)));
    s.c = F / 16 * cos2_alpha * (4 + F * (4 - 3 * cos2_alpha));
    return s;
}
__device__ __forceinline__ double arc(double sigma, double cos_2sm, double a, double b) {
    const double sin_s = sin(sigma), cos_s = cos(sigma);
    const double dsig = b * sin_s * (cos_2sm + b / 4 * (cos_s * (-1 + 2 * cos_2sm * cos_2sm) -
                                                        b / 6 * cos_2sm * (-3 + 4 * sin_s * sin_s) * (-3 + 4 * cos_2sm * cos_2sm)));
    return B * a * (sigma - dsig);
}
__device__ __forceinline__ double reduced_latitude(double lat_deg) { return atan((1.0 - F) * tan(lat_deg * (PI / 180.0))); }
__device__ __forceinline__ double meridian_arc(double lat_deg) {
    double U = fabs(reduced_latitude(lat_deg));
    if (fabs(lat_deg) >= 90.0) U = 0.5 * PI;
    const Series s = series(1.0);
    return arc(U, cos(U), s.a, s.b);
}
// leave reduced latitude U (>= 0) with azimuth a1 in [0, pi/2], travel until latitude U is reached again
__device__ __forceinline__ void symmetric(double U, double a1, double &L, double &len) {
    const double sinU = sin(U), cosU = cos(U), sin_a1 = sin(a1), cos_a1 = cos(a1);
    const double s1 = atan2(sinU, cosU * cos_a1);
    const double sigma = PI - 2.0 * s1;
    const double sin_alpha = cosU * sin_a1;
    const double cos2_alpha = 1.0 - sin_alpha * sin_alpha;
    const Series s = series(cos2_alpha);
    const double sin_s = sin(sigma), cos_s = cos(sigma);
    double omega = atan2(sin_s * sin_a1, cosU * cos_s - sinU * sin_s * cos_a1);
    if (omega < 0) omega += 2 * PI;
    const double cos_2sm = -1.0;
    L = omega - (1 - s.c) * F * sin_alpha * (sigma + s.c * sin_s * (cos_2sm + s.c * cos_s * (-1 + 2 * cos_2sm * cos_2sm)));
    len = arc(sigma, cos_2sm, s.a, s.b);
}
// lat, lon [deg] (lon folded to (-180, 180]) -> lat_m, lon_m, lon_off; quarter = meridian_arc(90)
struct Planar { double lat_m, lon_m, lon_off; };
__device__ __forceinline__ Planar planar(double la, double lo) {
    const double quarter = meridian_arc(90.0);
    const double arc_m = meridian_arc(la);
    const double over_pole = 2.0 * (quarter - arc_m);
    const double sgn_la = (la > 0) - (la < 0), sgn_lo = (lo > 0) - (lo < 0);
    const double dl = fabs(lo), U = fabs(reduced_latitude(la)), Ls = dl * (PI / 180.0);
    double a_lo = 0.0, a_hi = 0.5 * PI, L, len;
    for (int it = 0; it < 70; ++it) {
        const double mid = 0.5 * (a_lo + a_hi);
        symmetric(U, mid, L, len);
        if (L > Ls) a_lo = mid; else a_hi = mid;
    }
    symmetric(U, 0.5 * (a_lo + a_hi), L, len);
    double s = len;
    if (U < 1e-15 && Ls <= (1.0 - F) * PI) s = A * Ls;                    // the equator itself
    if (dl >= 180.0) s = over_pole;
    if (fabs(la) >= 90.0) s = 0.0;
    if (dl == 0.0) s = 0.0;
    if (la != la || lo != lo) s = __builtin_nan("");
    Planar p;
    p.lat_m = arc_m * sgn_la;
    p.lon_m = s * sgn_lo;
    p.lon_off = over_pole;
    return p;
}
}  // namespace geo

__global__ __launch_bounds__(BLOCK) void k_planar_metres(long long n, const double *__restrict__ lat, const double *__restrict__ lon,
                                                        double *__restrict__ lat_m, double *__restrict__ lon_m,
                                                        double *__restrict__ lon_off) {
    const long long i = (long long)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    const geo::Planar p = geo::planar(lat[i], lon[i]);
    lat_m[i] = p.lat_m;
    lon_m[i] = p.lon_m;
    lon_off[i] = p.lon_off;
}

// Target coordinates of the ocean-grid interpolation for point-wise targets (functions.py:998-1023), one target per thread:
// the longitude folded to (-180, 180], the planar lengths evaluated on (|lat|, |lon|) and given the signs of lat and lon -
// the arithmetic gauss_interp_fields applies to the distinct |lat| x |lon| of a mesh, so a mesh handed over point by point
// gets the same bits.  A target with land[i] > 0.7 (`land` may be null; a NaN fraction is not > 0.7) or a NaN coordinate is
// inactive: tx = ty = NaN, and the bisection is not run for it.
__global__ __launch_bounds__(BLOCK) void k_ocean_targets(long long n, const double *__restrict__ lat, const double *__restrict__ lon,
                                                        const double *__restrict__ land, double *__restrict__ tx,
                                                        double *__restrict__ ty) {
    const long long i = (long long)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    const double la = lat[i];
    double lo = lon[i];
    if (lo > 180.0) lo -= 360.0;
    double x = __builtin_nan(""), y = __builtin_nan("");
    if (!((land && land[i] > 0.7) || la != la || lo != lo)) {
        const geo::Planar p = geo::planar(fabs(la), fabs(lo));
        x = p.lat_m * (double)((la > 0) - (la < 0));
        y = p.lon_m * (double)((lo > 0) - (lo < 0));
    }
    tx[i] = x;
    ty[i] = y;
}

template <bool SWAP>
__global__ __launch_bounds__(BLOCK) void k_narrow_f64_f32(long long n2, long long n, const double *__restrict__ src, unsigned int *__restrict__ dst) {
    typedef double d2 __attribute__((ext_vector_type(2)));
    typedef unsigned int u2 __attribute__((ext_vector_type(2)));
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n2; i += stride) {
        const d2 v = __builtin_nontemporal_load(reinterpret_cast<const d2 *>(src) + i);
        u2 o;
        o.x = __float_as_uint((float)v.x); o.y = __float_as_uint((float)v.y);
        if (SWAP) { o.x = __builtin_bswap32(o.x); o.y = __builtin_bswap32(o.y); }
        __builtin_nontemporal_store(o, reinterpret_cast<u2 *>(dst) + i);
    }
    for (long long e = 2 * n2 + (long long)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += stride) {
        unsigned int o = __float_as_uint((float)src[e]);
        dst[e] = SWAP ? __builtin_bswap32(o) : o;
    }
}

// Placement probe (pgw_placement_probe): the access pattern of the column kernels with no arithmetic - one thread per column,
// blocks of 128 columns, `ns` read streams and `nd` write streams of (row, column) float64 arrays, two rows per step with the
// next step's rows requested one step ahead, streaming loads and stores.  What it measures: the rate this set of arrays gets
// WHERE hipMalloc put them - on an MI355X an array that is written while another one of the same stretch of physical memory
// is read gets 5.0-5.4 TB/s, arrays of different stretches 5.7-6.2 (tools/micro/pair_matrix.hip).
struct ProbeStreams { const double *src[4]; double *dst[4]; int ns, nd; };
__global__ __launch_bounds__(128) void k_placement_probe(long long rows, long long ncol, ProbeStreams s) {
    const long long c = (long long)blockIdx.x * 128 + threadIdx.x;
    if (c >= ncol) return;
    auto row_sum = [&](long long r) {
        double a = 0.0;
#pragma unroll
        for (int i = 0; i < 4; ++i) if (i < s.ns) a += __builtin_nontemporal_load(s.src[i] + r * ncol + c);
        return a;
    };
    auto row_put = [&](long long r, double v) {
#pragma unroll
        for (int i = 0; i < 4; ++i) if (i < s.nd) __builtin_nontemporal_store(v, s.dst[i] + r * ncol + c);
    };
    double a = row_sum(0), b = rows > 1 ? row_sum(1) : 0.0;
    long long r = 0;
    for (; r + 1 < rows; r += 2) {
        double a2 = 0.0, b2 = 0.0;
        if (r + 2 < rows) a2 = row_sum(r + 2);
        if (r + 3 < rows) b2 = row_sum(r + 3);
        row_put(r, a); row_put(r + 1, b);
        a = a2; b = b2;
    }
    if (r < rows) row_put(r, a);
}

// Byte-order conversion of a field (NetCDF classic data are big-endian): every 4- or 8-byte element of `src` is
// written byte-reversed to `dst` (in place allowed), 16 B per lane, grid-stride.  HBM-bound: 2 x n x W bytes.
template <int W>
__global__ __launch_bounds__(BLOCK) void k_byteswap(long long n16, long long n, const uint4 *src, uint4 *dst) {   // may alias
    const long long stride = (long long)gridDim.x * blockDim.x;
    typedef unsigned int u4 __attribute__((ext_vector_type(4)));
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n16; i += stride) {
        const u4 t = __builtin_nontemporal_load(reinterpret_cast<const u4 *>(src) + i);   // read once, written once
        uint4 v = make_uint4(t.x, t.y, t.z, t.w);
        if (W == 4) {
            v.x = __builtin_bswap32(v.x); v.y = __builtin_bswap32(v.y);
            v.z = __builtin_bswap32(v.z); v.w = __builtin_bswap32(v.w);
        } else {
            unsigned int a = __builtin_bswap32(v.y), b = __builtin_bswap32(v.x);
            unsigned int c = __builtin_bswap32(v.w), d = __builtin_bswap32(v.z);
            v.x = a; v.y = b; v.z = c; v.w = d;
        }
        { u4 o; o.x = v.x; o.y = v.y; o.z = v.z; o.w = v.w; __builtin_nontemporal_store(o, reinterpret_cast<u4 *>(dst) + i); }
    }
    // tail elements (n not a multiple of 16 / W) and the unaligned case (n16 == 0): element by element
    const long long done = n16 * (16 / W);
    for (long long e = done + (long long)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += stride) {
        if (W == 4) {
            ((unsigned int *)dst)[e] = __builtin_bswap32(((const unsigned int *)src)[e]);
        } else {
            ((unsigned long long *)dst)[e] = __builtin_bswap64(((const unsigned long long *)src)[e]);
        }
    }
}

// the device logarithms over an array (diagnostic entries pgw_test_log, pgw_test_log_table, pgw_test_log_f3, pgw_test_log_dd;
// tests compare them with the exact logarithm): which = 0 pgw_log, 1 pgw_log_tab, 2 pgw_log_f3, 3 pgw_log_dd
__global__ void k_test_log(long long n, const double *__restrict__ in, double *__restrict__ out, int which) {
    __shared__ double s_tab[2 * LOG_TABLE_N];
    stage_log_table(s_tab, blockDim.x);
    __syncthreads();
    long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const double x = in[i];
    out[i] = which == 1 ? pgw_log_tab(x, s_tab) : which == 2 ? pgw_log_f3(x) : which == 3 ? pgw_log_dd(x) : pgw_log(x);
}

// pgw_exp and the device library's exp over an array (diagnostic entry pgw_test_exp): out[i] = pgw_exp(in[i]),
// ref[i] = exp(in[i])
__global__ void k_test_exp(long long n, const double *__restrict__ in, double *__restrict__ out, double *__restrict__ ref) {
    long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) { out[i] = pgw_exp(in[i]); ref[i] = exp(in[i]); }
}

// pgw_exp_finite / pgw_exp_reduced over an array (diagnostic entries pgw_test_exp_finite, pgw_test_exp_reduced; tests compare
// them with pgw_exp)
__global__ void k_test_exp_finite(long long n, const double *__restrict__ in, double *__restrict__ out, int reduced) {
    long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = reduced ? pgw_exp_reduced(in[i]) : pgw_exp_finite(in[i]);
}

// RELHUM of a float32 ERA state in reference-dtype mode (diagnostic entry pgw_test_rh_f32): the fast form the quad kernel
// uses and the literal expression, side by side
__global__ void k_test_rh_f32(long long n, const float *__restrict__ hus, const double *__restrict__ pa,
                              const float *__restrict__ ta, double *__restrict__ out, double *__restrict__ lit,
                              float *__restrict__ es, float *__restrict__ es_lit) {
    long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) {
        out[i] = q_to_rh_f32(hus[i], pa[i], ta[i]);
        lit[i] = q_to_rh_f32_literal(hus[i], pa[i], ta[i]);
        es[i] = esat_mixed_f32(ta[i]);
        es_lit[i] = esat_mixed_f32_literal(ta[i]);
    }
}

// SharedDivisor over arrays (diagnostic entry pgw_test_shared_div; tests compare it with IEEE division)
__global__ void k_test_shared_div(long long n, const double *__restrict__ num, const double *__restrict__ den,
                                  double *__restrict__ out) {
    long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = (den[i] == 100.0) ? div_by_100(num[i]) : SharedDivisor(den[i]).divide(num[i]);
}

// ln() of a small table with the device log (so table entries and per-column logs come from
// the same implementation)
__global__ void k_log_table(int n, const double *in, double *out) {
    __shared__ double s_tab[2 * LOG_TABLE_N];
    stage_log_table(s_tab, blockDim.x);
    __syncthreads();
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = pgw_log_tab(in[i], s_tab);
}

// =====================================================================================
// c1  hydrostatic check: geopotential on a list of pressure levels       functions.py:128-189, once per level
// phi(p) = integ_geopot(ak + PS * bk, FIS, T, QV, level1, p_ref = p) for every p of a level list, in ONE walk of the
// column from the surface up; for two states (ERA5 and PGW: own PS, T, QV; shared FIS and coefficients) the difference
// phi_b - phi_a, and with a zg record pair phi_error = (phi_b - phi_a) - g * zg_delta (step_03:298 on every level).
// float64 arithmetic on the stored values (the REF = false forms), every logarithm from pgw_log_tab - half levels and
// targets alike (GeoTargets::lnp is made by k_log_table), so a target that equals a half-level pressure has a zero
// logarithm difference and gets phi_hl[k*] bit for bit (p == p_hl[N]: FIS).
//
// Rule.  k* = the half level with the smallest non-negative fix_p(p_hl) - p, ties to the lowest index (:160-163); the
// value is phi_hl[k*] - Rd Tv[k* - 1] (ln p - ln p_hl[k*]) (:174-179).  NaN, and the column counted for that level,
// where no half level has p_hl >= p (the reference raises, :162-165) and where k* = 0 (level 0 has no layer above it:
// the reference's KeyError, :176; cannot happen for ak[0] = 0, because the host refuses p <= 1e-4).
// A wave whose columns all have ascending half-level pressures in every state (ps >= Levels::ps_mono_min; false for
// NaN) walks once: the targets are held in descending pressure, a column's position j in that list only moves forward,
// and layer l (between half levels l + 1 and l) emits every target with p_hl[l] < p <= p_hl[l + 1] - for which k* = l + 1 -
// from the running phi, exactly geo_layer's capture and geo_finish's expression.  Any other wave takes the general form:
// per target one full scan with geo_layer's k* tracking (dmin, `<=` for the ties), S scans in all.  Both forms do the
// same operations on the same values for an ascending column: same bits.
//
// Two states meet in the output row itself: a state that reaches target j first stores its own value there, the other
// one reads it back and stores the result (same thread, same address: program order).  MEET walks both states level by
// level in one loop (162 VGPRs, 3 waves per SIMD); the two-walk form walks state a, then state b, in the same launch (116
// VGPRs, 4 waves) and is what functions.GEOPOT_PLEV_FORM selects: the only form that beat two one-state launches plus a
// subtraction for float64 and for float32 level arrays.  DESIGN.md section 4 has the times.
// =====================================================================================
struct GeoTargets {
    double p[MAX_PLEV];      // descending pressure
    double lnp[MAX_PLEV];    // pgw_log_tab of them
    int row[MAX_PLEV];       // output row of each: the caller's order
    int n;
};
struct ZgDelta {             // bracketing zg records (time, S, ncol) in the caller's level order; b == nullptr: none
    const void *b, *a;       // a == nullptr: the instant is record b
    int f32;                 // storage type of both
    double x_hi, x_new, g;
    __device__ __forceinline__ double gdz(long long off) const {
        if (f32) return DeltaSrc<float>{(const float *)b, (const float *)a, x_hi, x_new}.get(off) * g;
        return DeltaSrc<double>{(const double *)b, (const double *)a, x_hi, x_new}.get(off) * g;
    }
};
constexpr int GEOPLEV_U = 4;
enum { GEO_PLAIN = 0, GEO_COMBINE = 1, GEO_MEET = 2 };

// One target's value leaves the walk.  PLAIN: stored.  COMBINE: the row holds state a's value, this is state b's.
// MEET: `other_done` says whether the other state has been here.
template <int MODE>
__device__ __forceinline__ void geo_emit(double val, int s, bool other_done, long long idx, int row, bool live, const ZgDelta &zg,
                                         double *out, unsigned int *s_cnt) {
    if (!live) return;
    if (MODE == GEO_PLAIN || (MODE == GEO_MEET && !other_done)) {
        out[idx] = val;
        if (MODE == GEO_PLAIN && s_cnt && val != val) atomicAdd(&s_cnt[row], 1u);      // s_cnt == nullptr: a value that waits
        return;
    }
    const double prev = out[idx];
    double r = (MODE == GEO_COMBINE || s == 1) ? val - prev : prev - val;          // phi_b - phi_a
    if (zg.b) r = r - zg.gdz(idx);                                                 // step_03:298
    out[idx] = r;
    if (r != r) atomicAdd(&s_cnt[row], 1u);
}

// The walk of NSW states of one column (ascending half-level pressures) through the descending targets
template <int NSW, int MODE, typename TLA, typename TLB>
__device__ __forceinline__ void geo_walk(const LevTab &lt, int N, int S, long long ncol, const double *s_p, const double *s_lnp,
                                         const int *s_row, const double *s_lnhl, const TLA *__restrict__ ta0, const TLA *__restrict__ q0,
                                         const TLB *__restrict__ ta1, const TLB *__restrict__ q1, const double (&ps)[NSW], double z,
                                         long long obase, bool live, const ZgDelta &zg, double *out, unsigned int *s_cnt) {
    constexpr int U = GEOPLEV_U;
    double phi[NSW], p_lo[NSW], lnp_lo[NSW];
    double pn[NSW];                            // the target at j: read again only after an emit (s_p[S] = -inf ends the list)
    int j[NSW];
    const double nan = __builtin_nan("");
    auto emit = [&](int s, double val) {
        const int row = s_row[j[s]];
        geo_emit<MODE>(val, s, NSW == 2 && j[NSW - 1 - s] > j[s], obase + (long long)row * ncol, row, live, zg, out, s_cnt);
        j[s] += 1;
        pn[s] = s_p[j[s]];
    };
    {
        const double akN = lt.ak[N], bkN = lt.bk[N];
#pragma unroll
        for (int s = 0; s < NSW; ++s) {
            phi[s] = z;
            p_lo[s] = fix_p(akN + ps[s] * bkN);
            lnp_lo[s] = pgw_log_tab(p_lo[s], lt.logtab);
            j[s] = 0;
            pn[s] = s_p[0];
        }
    }
#pragma unroll
    for (int s = 0; s < NSW; ++s)
        while (pn[s] > p_lo[s]) emit(s, nan);                                      // below the surface half level
    double tn[U][NSW], qn[U][NSW];
    auto request = [&](int l0) {                                                   // rows l0, l0 - 1, ... (clamped at 0)
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const long long lu = (l0 - u) > 0 ? (l0 - u) : 0;
            tn[u][0] = (double)__builtin_nontemporal_load(ta0 + lu * ncol);
            qn[u][0] = (double)__builtin_nontemporal_load(q0 + lu * ncol);
            if constexpr (NSW == 2) {
                tn[u][1] = (double)__builtin_nontemporal_load(ta1 + lu * ncol);
                qn[u][1] = (double)__builtin_nontemporal_load(q1 + lu * ncol);
            }
        }
    };
    request(N - 1);
    for (int l = N - 1; l >= 0; l -= U) {
        double t[U][NSW], q[U][NSW];
#pragma unroll
        for (int u = 0; u < U; ++u)
#pragma unroll
            for (int s = 0; s < NSW; ++s) { t[u][s] = tn[u][s]; q[u][s] = qn[u][s]; }
        if (l - U >= 0) request(l - U);
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int lc = l - u;
            if (lc >= 0) {
                const double a = lt.ak[lc], b = lt.bk[lc];
                const bool pure = b == 0.0;                                        // the same pressure in every column: ak
                const double lna = s_lnhl[lc];
#pragma unroll
                for (int s = 0; s < NSW; ++s) {
                    const double rtv = CON_RD * (t[u][s] * (1 + 0.61 * q[u][s]));  // :144, :150
                    const double p_hi = fix_p(a + ps[s] * b);                      // :135
                    const double lnp_hi = pure ? lna : pgw_log_tab(p_hi, lt.logtab);
                    while (pn[s] > p_hi) emit(s, phi[s] - rtv * (s_lnp[j[s]] - lnp_lo[s]));    // k* = lc + 1, :174-179
                    phi[s] = phi[s] + rtv * (lnp_lo[s] - lnp_hi);                  // :149-152
                    p_lo[s] = p_hi; lnp_lo[s] = lnp_hi;
                }
            }
        }
    }
#pragma unroll
    for (int s = 0; s < NSW; ++s)
        while (j[s] < S) emit(s, nan);                                             // k* = 0
}

// One target, one state, any column: geo_layer's scan and geo_finish's expression with the target's tabulated logarithm
template <typename TL>
__device__ __forceinline__ double geo_general(const LevTab &lt, int N, long long ncol, const TL *__restrict__ ta, const TL *__restrict__ hus,
                                              double ps, double z, double p, double lnp) {
    GeoAcc acc;
    geo_init(acc, z, lt.ak[N] + ps * lt.bk[N], lt.logtab);
    for (int l = N - 1; l >= 0; --l) {
        const double t = (double)ta[(long long)l * ncol], q = (double)hus[(long long)l * ncol];
        geo_layer<false, true>(acc, l, CON_RD * (t * (1 + 0.61 * q)), lt.ak[l] + ps * lt.bk[l], p, lt.logtab);
    }
    const double d = acc.p_lo - p;                                                 // candidate k = 0
    if (d >= 0 && d <= acc.dmin) acc.kstar = 0;
    if (acc.kstar <= 0) return __builtin_nan("");
    return acc.phi_s - acc.rtv_s * (lnp - acc.lnp_s);
}

// T2: storage type of PS (both states) and FIS; TLA / TLB: of the level arrays of state a / b.  NS = 1: out = phi_a;
// NS = 2: phi_b - phi_a, minus g * zg_delta when zg.b is set.  out (ntime, S, ncol) float64 in the caller's level order;
// nan_count[row] += NaN columns of that row (integer adds: the same total in any order).
template <typename T2, typename TLA, typename TLB, int NS, bool MEET>
__global__ __launch_bounds__(BLOCK) void k_geopot_plev(GeoTargets gt, Levels lv, int ntime, long long ncol,
                                                       const T2 *__restrict__ FIS, const T2 *__restrict__ PS_a,
                                                       const TLA *__restrict__ T_a, const TLA *__restrict__ QV_a,
                                                       const T2 *__restrict__ PS_b, const TLB *__restrict__ T_b,
                                                       const TLB *__restrict__ QV_b, ZgDelta zg, double *out,
                                                       unsigned long long *__restrict__ nan_count) {
    __shared__ double s_lev[LEVTAB_DOUBLES];
    __shared__ double s_p[MAX_PLEV + 1], s_lnp[MAX_PLEV + 1];
    __shared__ int s_row[MAX_PLEV + 1];
    __shared__ unsigned int s_cnt[MAX_PLEV];
    __shared__ double s_lnhl[MAX_NLEV + 1];    // ln fix_p(ak[l]): the logarithm of a pure-pressure half level (bk[l] = 0), once per block
    const int S = gt.n, N = lv.nlev;
    for (int i = threadIdx.x; i <= MAX_PLEV; i += BLOCK) {
        const bool in = i < S;                 // behind the list: a pressure no half level lies below
        s_p[i] = in ? gt.p[i] : -__builtin_inf(); s_lnp[i] = in ? gt.lnp[i] : 0.0; s_row[i] = in ? gt.row[i] : 0;
        if (i < MAX_PLEV) s_cnt[i] = 0u;
    }
    LevTab lt = stage_levels<true, false>(lv, s_lev, BLOCK);                      // synchronises
    for (int i = threadIdx.x; i <= N; i += BLOCK) s_lnhl[i] = pgw_log_tab(fix_p(lt.ak[i]), lt.logtab);
    __syncthreads();
    const long long ntot = (long long)ntime * ncol;
    long long g = (long long)blockIdx.x * BLOCK + threadIdx.x;
    const bool live = g < ntot;
    if (!live) g = ntot - 1;                  // idle lanes of the last block shadow its last column and store nothing
    const long long t = g / ncol, c = g - t * ncol;
    const long long lbase = t * N * ncol + c, obase = t * S * ncol + c;
    const double z = (double)FIS[g];
    double ps[NS];
    ps[0] = (double)PS_a[g];
    if constexpr (NS == 2) ps[1] = (double)PS_b[g];
    constexpr double DBL_MAX_ = 1.7976931348623157e308;           // an infinite PS ascends nowhere (inf * 0 on the pure-pressure levels)
    bool mono = ps[0] >= lv.ps_mono_min && ps[0] <= DBL_MAX_;
    if constexpr (NS == 2) mono = mono && ps[1] >= lv.ps_mono_min && ps[1] <= DBL_MAX_;
    if (__all(mono)) {
        if constexpr (NS == 1) {
            geo_walk<1, GEO_PLAIN, TLA, TLA>(lt, N, S, ncol, s_p, s_lnp, s_row, s_lnhl, T_a + lbase, QV_a + lbase, nullptr, nullptr, ps, z,
                                             obase, live, zg, out, s_cnt);
        } else if constexpr (MEET) {
            geo_walk<2, GEO_MEET, TLA, TLB>(lt, N, S, ncol, s_p, s_lnp, s_row, s_lnhl, T_a + lbase, QV_a + lbase, T_b + lbase, QV_b + lbase,
                                            ps, z, obase, live, zg, out, s_cnt);
        } else {
            const double pa[1] = {ps[0]}, pb[1] = {ps[1]};
            geo_walk<1, GEO_PLAIN, TLA, TLA>(lt, N, S, ncol, s_p, s_lnp, s_row, s_lnhl, T_a + lbase, QV_a + lbase, nullptr, nullptr, pa, z,
                                             obase, live, zg, out, nullptr);
            geo_walk<1, GEO_COMBINE, TLB, TLB>(lt, N, S, ncol, s_p, s_lnp, s_row, s_lnhl, T_b + lbase, QV_b + lbase, nullptr, nullptr, pb, z,
                                               obase, live, zg, out, s_cnt);
        }
    } else {
        for (int j = 0; j < S; ++j) {
            const int row = s_row[j];
            const long long idx = obase + (long long)row * ncol;
            double r = geo_general<TLA>(lt, N, ncol, T_a + lbase, QV_a + lbase, ps[0], z, s_p[j], s_lnp[j]);
            if constexpr (NS == 2) {
                r = geo_general<TLB>(lt, N, ncol, T_b + lbase, QV_b + lbase, ps[1], z, s_p[j], s_lnp[j]) - r;
                if (zg.b) r = r - zg.gdz(idx);
            }
            if (live) {
                out[idx] = r;
                if (r != r) atomicAdd(&s_cnt[row], 1u);
            }
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < S; i += BLOCK)
        if (s_cnt[i]) atomicAdd(&nan_count[i], (unsigned long long)s_cnt[i]);
}

// =====================================================================================
// c2  per-row statistics of a (nrow, ncol) float64 array, NaN skipped: count, sum, sum of squares, max |x|
// Block (bx, row) takes the columns bx * BLOCK + tid, + gridDim.x * BLOCK, ... in that order, the block folds its 256
// partials with a fixed tree, and writes part[(row * gridDim.x + bx) * 4 ..]; the host entry adds the blocks of a row in
// the order of bx.  The grid depends on the shape alone: two calls give the same bits.
// =====================================================================================
__global__ __launch_bounds__(BLOCK) void k_level_stats(long long ncol, const double *__restrict__ x, double *__restrict__ part) {
    __shared__ double s_red[4][BLOCK];
    const double *r = x + (long long)blockIdx.y * ncol;
    double cnt = 0.0, sum = 0.0, sq = 0.0, mx = 0.0;
    for (long long i = (long long)blockIdx.x * BLOCK + threadIdx.x; i < ncol; i += (long long)gridDim.x * BLOCK) {
        const double v = r[i];
        if (v == v) { cnt += 1.0; sum += v; sq += v * v; mx = fmax(mx, fabs(v)); }
    }
    s_red[0][threadIdx.x] = cnt; s_red[1][threadIdx.x] = sum; s_red[2][threadIdx.x] = sq; s_red[3][threadIdx.x] = mx;
    __syncthreads();
    for (int h = BLOCK / 2; h > 0; h >>= 1) {
        if ((int)threadIdx.x < h) {
            s_red[0][threadIdx.x] += s_red[0][threadIdx.x + h];
            s_red[1][threadIdx.x] += s_red[1][threadIdx.x + h];
            s_red[2][threadIdx.x] += s_red[2][threadIdx.x + h];
            s_red[3][threadIdx.x] = fmax(s_red[3][threadIdx.x], s_red[3][threadIdx.x + h]);
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        double *o = part + ((long long)blockIdx.y * gridDim.x + blockIdx.x) * 4;
        o[0] = s_red[0][0]; o[1] = s_red[1][0]; o[2] = s_red[2][0]; o[3] = s_red[3][0];
    }
}

// =====================================================================================
// c3  delta check: T, RH, U, V of an ERA5-like state on a list of pressure levels       functions.py:107-116, 511-580, 288-292
// Per column and state: pa[k] = akm[k] + PS * bkm[k] (product, then sum), RH[k] = q_to_rh(QV[k], pa[k], T[k]), and for X in
// (T, RH, U, V) X(p) = interp_extrap_1d(ln pa, X, ln p, 'nan'): the first k with ln pa[k] == ln p or > ln p; equal gives
// X[k], k = 0 with "greater" and no such k give NaN, else X[k-1] + (ln p - ln pa[k-1]) * (X[k] - X[k-1]) / (ln pa[k] -
// ln pa[k-1]) in this order.  float64 arithmetic on the stored values, every logarithm from pgw_log_tab (equal pressures
// have equal logarithms): what pgw_specific_to_relative_humidity_hybrid + four pgw_interp_hybrid_to_plev launches
// (F64 -> F64, PGW_EXTRAP_NAN) give on widened arrays, bit for bit.  A column with pa[N-1] < pa[0] gives NaN everywhere.
//
// One thread per column walks the model levels once per state; the targets are held ascending, so the column's position
// in the list only moves forward, and the level k that ends a bracket emits every target in it for all four variables
// from ONE pair of logarithms (the divisions share their denominator: the compiler keeps one reciprocal refinement).
// RH is formed only for the two levels of a bracket that holds a target: at most 2 S e_sat evaluations per state, not N.
// The leading levels with bkm = 0 take their logarithm from a per-block table like k_hybrid_to_plev.  The next level's
// four loads are in flight while the current level is worked on.
// Two states (NS = 2): state a's walk stores X_a in the output rows, state b's walk reads them back (same thread, same
// address: program order) and stores change = X_b - X_a, and with the record pairs error = change - delta where
// p < ps_hist, else NaN; delta and ps_hist are interpolated in time like load_delta (DeltaSrc::get), each on its own axis.
// out / out_error (4, ntime, S, ncol) float64 in the order (ta, hur, ua, va), rows in the caller's level order.
// =====================================================================================
struct PlevRecords {         // bracketing records of the four deltas (ntime, S, ncol) and of ps_hist (ntime, ncol); b[0] == nullptr: none
    const void *b[4], *a[4]; // a[v] == nullptr: the instant is record b[v]
    const void *ps_b, *ps_a;
    double x_hi[5], x_new[5];
    int f32;                 // storage type of all ten
    __device__ __forceinline__ double get(int v, long long off) const {
        if (f32) return DeltaSrc<float>{(const float *)b[v], (const float *)a[v], x_hi[v], x_new[v]}.get(off);
        return DeltaSrc<double>{(const double *)b[v], (const double *)a[v], x_hi[v], x_new[v]}.get(off);
    }
    __device__ __forceinline__ double ps_hist(long long off) const {
        if (f32) return DeltaSrc<float>{(const float *)ps_b, (const float *)ps_a, x_hi[4], x_new[4]}.get(off);
        return DeltaSrc<double>{(const double *)ps_b, (const double *)ps_a, x_hi[4], x_new[4]}.get(off);
    }
};

// The walk of one state.  COMBINE = false: X is stored (streaming when nothing reads it back: NT).  COMBINE = true: the
// rows hold state a's values; change and, with records, error are stored.
template <bool COMBINE, bool NT, typename TL, typename O>
__device__ __forceinline__ void state_walk(const LevTab &lt, int N, int S, int n_pure, const double *s_lx, const double *s_p,
                                           const int *s_row, const double *s_lap, const TL *__restrict__ Tl,
                                           const TL *__restrict__ Ql, const TL *__restrict__ Ul, const TL *__restrict__ Vl,
                                           double ps, O lbase, O rowb_in, O obase, O rowb_out, O varb_out, long long rbase,
                                           long long ncol, double psh, const PlevRecords &rec, double *out, double *out_error) {
    const double nan = __builtin_nan("");
    int jt = 0;
    double lx = s_lx[0];                                                           // s_lx[S] = NaN ends the list
    auto emit = [&](const double (&val)[4]) {
        const int row = s_row[jt];
        const O o = obase + (O)row * rowb_out;
#pragma unroll
        for (int v = 0; v < 4; ++v) {
            const O ov = o + (O)v * varb_out;
            if constexpr (!COMBINE) {
                if (NT) st_off_nt<double, O>(out, ov, val[v]);
                else st_off<double, O>(out, ov, val[v]);
            } else {
                const double change = val[v] - ld_off<double, O>(out, ov);         // X_b - X_a
                st_off_nt<double, O>(out, ov, change);
                if (out_error) {
                    const double e = (s_p[jt] < psh) ? change - rec.get(v, rbase + (long long)row * ncol) : nan;
                    st_off_nt<double, O>(out_error, ov, e);
                }
            }
        }
        ++jt;
        lx = s_lx[jt];
    };
    const bool ps_finite = (ps - ps == 0.0);                                       // 0 * ps = 0: not for NaN / inf
    const double pa_top = lt.akm[0] + ps * lt.bkm[0], pa_bot = lt.akm[N - 1] + ps * lt.bkm[N - 1];
    const int nwalk = (pa_bot < pa_top) ? 0 : N;                                   // such a column: NaN on every level
    auto ld = [&](const TL *p, int k) { return ld_off_nt<TL, O>(p, lbase + (O)k * rowb_in); };
    TL nt_ = ld(Tl, 0), nq_ = ld(Ql, 0), nu_ = ld(Ul, 0), nv_ = ld(Vl, 0);
    double xm = 0, pam = 0, tm = 0, qm = 0, um = 0, vm = 0;
    for (int k = 0; k < nwalk; ++k) {
        const double t = (double)nt_, q = (double)nq_, u = (double)nu_, w = (double)nv_;
        const int kn = k + 1 < N ? k + 1 : N - 1;
        nt_ = ld(Tl, kn); nq_ = ld(Ql, kn); nu_ = ld(Ul, kn); nv_ = ld(Vl, kn);
        const double pa = lt.akm[k] + ps * lt.bkm[k];
        const double x = (k < n_pure && ps_finite) ? s_lap[k] : pgw_log_tab(no_speculate(pa), lt.logtab);
        if (x == lx || x > lx) {                                                   // level k is the first at or past target jt
            if (k == 0) { pam = pa; tm = t; qm = q; }
            const double rh = q_to_rh(q, pa, t), rhm = q_to_rh(qm, pam, tm);
            const double dx = x - xm;
            do {
                double val[4];
                if (x == lx) { val[0] = t; val[1] = rh; val[2] = u; val[3] = w; }  // :540-543
                else if (k == 0) { val[0] = val[1] = val[2] = val[3] = nan; }      // above the top full level, 'nan'
                else {                                                             // :575-578
                    const double f = lx - xm;
                    val[0] = tm + f * (t - tm) / dx;
                    val[1] = rhm + f * (rh - rhm) / dx;
                    val[2] = um + f * (u - um) / dx;
                    val[3] = vm + f * (w - vm) / dx;
                }
                emit(val);
            } while (x == lx || x > lx);
            if (jt >= S) break;
        }
        xm = x; pam = pa; tm = t; qm = q; um = u; vm = w;
    }
    const double none[4] = {nan, nan, nan, nan};
    while (jt < S) emit(none);                                                     // below the lowest full level
}

// T2: storage type of PS of both states; TLA / TLB: of the level arrays of state a / b; O: byte-offset type of every array
template <typename T2, typename TLA, typename TLB, int NS, typename O>
__global__ __launch_bounds__(BLOCK) void k_state_plev(Levels lv, int ntime, int S, long long ncol, const double *__restrict__ plev_sorted,
                                                      const int *__restrict__ rows, const T2 *__restrict__ PS_a,
                                                      const TLA *__restrict__ T_a, const TLA *__restrict__ QV_a,
                                                      const TLA *__restrict__ U_a, const TLA *__restrict__ V_a,
                                                      const T2 *__restrict__ PS_b, const TLB *__restrict__ T_b,
                                                      const TLB *__restrict__ QV_b, const TLB *__restrict__ U_b,
                                                      const TLB *__restrict__ V_b, PlevRecords rec, double *out, double *out_error) {
    __shared__ double s_lev[LEVTAB_DOUBLES];
    __shared__ double s_p[MAX_PLEV_WIDE + 1], s_lx[MAX_PLEV_WIDE + 1];            // ascending pressure, and its logarithm
    __shared__ int s_row[MAX_PLEV_WIDE + 1];
    __shared__ double s_lap[MAX_NLEV];                                            // ln akm[k] of the leading levels with bkm = 0
    __shared__ int s_npure;
    const int N = lv.nlev;
    if (threadIdx.x == 0) s_npure = N;
    LevTab lt = stage_levels<false, true>(lv, s_lev, BLOCK);                      // synchronises
    for (int i = threadIdx.x; i <= MAX_PLEV_WIDE; i += BLOCK) {
        const bool in = i < S;
        const double p = in ? plev_sorted[i] : __builtin_nan("");
        s_p[i] = p; s_lx[i] = in ? pgw_log_tab(p, lt.logtab) : p; s_row[i] = in ? rows[i] : 0;
    }
    for (int i = threadIdx.x; i < N; i += BLOCK) {
        s_lap[i] = pgw_log_tab(lt.akm[i], lt.logtab);
        if (!(lt.bkm[i] == 0.0)) atomicMin(&s_npure, i);
    }
    __syncthreads();
    const int n_pure = s_npure;
    const long long g = (long long)blockIdx.x * BLOCK + threadIdx.x;
    if (g >= (long long)ntime * ncol) return;
    const long long t = g / ncol, c = g - t * ncol;
    const O rowb_out = (O)((unsigned long long)ncol * sizeof(double));
    const O varb_out = (O)((unsigned long long)ntime * S * ncol * sizeof(double));
    const O obase = (O)((unsigned long long)(t * S * ncol + c) * sizeof(double));
    const long long rbase = t * S * ncol + c;
    const double ps_a = (double)PS_a[g];
    {
        const O rowb = (O)((unsigned long long)ncol * sizeof(TLA)), lbase = (O)((unsigned long long)(t * N * ncol + c) * sizeof(TLA));
        state_walk<false, NS == 1, TLA, O>(lt, N, S, n_pure, s_lx, s_p, s_row, s_lap, T_a, QV_a, U_a, V_a, ps_a, lbase, rowb, obase,
                                           rowb_out, varb_out, rbase, ncol, 0.0, rec, out, nullptr);
    }
    if constexpr (NS == 2) {
        const O rowb = (O)((unsigned long long)ncol * sizeof(TLB)), lbase = (O)((unsigned long long)(t * N * ncol + c) * sizeof(TLB));
        const double psh = out_error ? rec.ps_hist(g) : 0.0;                       // NaN: p < psh is false everywhere
        state_walk<true, true, TLB, O>(lt, N, S, n_pure, s_lx, s_p, s_row, s_lap, T_b, QV_b, U_b, V_b, (double)PS_b[g], lbase, rowb,
                                       obase, rowb_out, varb_out, rbase, ncol, psh, rec, out, out_error);
    }
}


// =====================================================================================
// a10b  bilinear regridding from curvilinear / rotated source grids       functions.py:797-810
// =====================================================================================
// What `xe.Regridder(ds_in, ds_era5, "bilinear", periodic=...)` asks ESMF for, stated natively: bilinear weights on the unit
// sphere in 3-D Cartesian space, a cell edge being the straight chord between its corners (ESMF's default line type for the
// non-conservative methods).  Two phases like a Regridder: k_cell_locate (geometry, once per grid pair) and k_regrid_sparse
// (every plane).  Preconditions: cells are convex and smaller than a hemisphere; concave cells are not detected.
//
// Nodes X[j*nx + i] and targets P are unit vectors the host forms in numpy; the kernels do no trigonometry and no square
// root, so every value below is IEEE + - * / in the order written (contraction is off) and numpy restates it bit for bit
// (locate_statement / apply_statement of tests/test_regrid_curvilinear_host.py; tests/test_regrid_curvilinear_hip.py compares).
//
//   det3(a, b, c) = ((a0 * (b1*c2 - b2*c1)) - (a1 * (b0*c2 - b2*c0))) + (a2 * (b0*c1 - b1*c0))
//
// Quad (A, B, C, D), patch p(s,t) = A + s(B-A) + t(D-A) + s t E, E = ((A - B) + C) - D.  Newton on p(s,t) - r P = 0 from
// s = t = 0.5, r = 1, at most CELL_NEWTON_MAX steps:
//   F  = (((A + s*ab) + t*ad) + (s*t)*E) - r*P           ab = B - A, ad = D - A
//   c1 = ab + t*E, c2 = ad + s*E, c3 = -P, det = det3(c1, c2, c3)          reject: det == 0 or not finite
//   ds = det3(F, c2, c3) / det, dt = det3(c1, F, c3) / det, dr = det3(c1, c2, F) / det;  s -= ds, t -= dt, r -= dr
//   reject: s, t or r not finite;  converged: |ds| <= 1e-14 and |dt| <= 1e-14
// reject: not converged, r <= 0, s or t outside [-1e-10, 1 + 1e-10].  Clamp s, t to [0, 1];
// weights (A, B, C, D) = (1-s)*(1-t), s*(1-t), s*t, (1-s)*t.
//
// Cap triangle (N, X1, X2):  e1 = X1 - N, e2 = X2 - N, c3 = -P, rhs = -N, det = det3(e1, e2, c3) (reject as above),
//   u = det3(rhs, e2, c3) / det, v = det3(e1, rhs, c3) / det, r = det3(e1, e2, rhs) / det
// reject: not finite, u or v < -1e-10, u + v > 1 + 1e-10, r <= 0.  Clamp: u = min(max(u, 0), 1), v = min(max(v, 0), 1 - u);
// weights (N, X1, X2) = (1 - u) - v, u, v.
constexpr int CELL_NEWTON_MAX = 20;
constexpr double CELL_STEP_TOL = 1e-14, CELL_ACCEPT_TOL = 1e-10;

struct Vec3 { double x, y, z; };
__device__ __forceinline__ Vec3 v3_load(const double *__restrict__ p, long long i) { return Vec3{p[3 * i], p[3 * i + 1], p[3 * i + 2]}; }
__device__ __forceinline__ Vec3 v3_sub(const Vec3 &a, const Vec3 &b) { return Vec3{a.x - b.x, a.y - b.y, a.z - b.z}; }
__device__ __forceinline__ Vec3 v3_add(const Vec3 &a, const Vec3 &b) { return Vec3{a.x + b.x, a.y + b.y, a.z + b.z}; }
__device__ __forceinline__ Vec3 v3_scale(double s, const Vec3 &a) { return Vec3{s * a.x, s * a.y, s * a.z}; }
__device__ __forceinline__ Vec3 v3_neg(const Vec3 &a) { return Vec3{-a.x, -a.y, -a.z}; }
__device__ __forceinline__ double det3(const Vec3 &a, const Vec3 &b, const Vec3 &c) {
    return ((a.x * (b.y * c.z - b.z * c.y)) - (a.y * (b.x * c.z - b.z * c.x))) + (a.z * (b.x * c.y - b.y * c.x));
}
__device__ __forceinline__ bool finite_d(double x) { return fabs(x) <= 1.7976931348623157e308; }    // false for NaN

__device__ __forceinline__ bool cell_solve_quad(const Vec3 &A, const Vec3 &B, const Vec3 &Cc, const Vec3 &D, const Vec3 &P,
                                                double (&w)[4]) {
    const Vec3 ab = v3_sub(B, A), ad = v3_sub(D, A), E = v3_sub(v3_add(v3_sub(A, B), Cc), D), c3 = v3_neg(P);
    double s = 0.5, t = 0.5, r = 1.0;
    bool conv = false;
    for (int it = 0; it < CELL_NEWTON_MAX; ++it) {
        const Vec3 F = v3_sub(v3_add(v3_add(v3_add(A, v3_scale(s, ab)), v3_scale(t, ad)), v3_scale(s * t, E)), v3_scale(r, P));
        const Vec3 c1 = v3_add(ab, v3_scale(t, E)), c2 = v3_add(ad, v3_scale(s, E));
        const double det = det3(c1, c2, c3);
        if (det == 0.0 || !finite_d(det)) return false;
        const double ds = det3(F, c2, c3) / det, dt = det3(c1, F, c3) / det, dr = det3(c1, c2, F) / det;
        s = s - ds; t = t - dt; r = r - dr;
        if (!(finite_d(s) && finite_d(t) && finite_d(r))) return false;
        if (fabs(ds) <= CELL_STEP_TOL && fabs(dt) <= CELL_STEP_TOL) { conv = true; break; }
    }
    if (!conv) return false;
    if (!(r > 0.0)) return false;
    if (!(s >= -CELL_ACCEPT_TOL && s <= 1.0 + CELL_ACCEPT_TOL && t >= -CELL_ACCEPT_TOL && t <= 1.0 + CELL_ACCEPT_TOL)) return false;
    s = s < 0.0 ? 0.0 : (s > 1.0 ? 1.0 : s);
    t = t < 0.0 ? 0.0 : (t > 1.0 ? 1.0 : t);
    const double os = 1.0 - s, ot = 1.0 - t;
    w[0] = os * ot; w[1] = s * ot; w[2] = s * t; w[3] = os * t;
    return true;
}

__device__ __forceinline__ bool cell_solve_tri(const Vec3 &N, const Vec3 &X1, const Vec3 &X2, const Vec3 &P, double (&w)[4]) {
    const Vec3 e1 = v3_sub(X1, N), e2 = v3_sub(X2, N), c3 = v3_neg(P), rhs = v3_neg(N);
    const double det = det3(e1, e2, c3);
    if (det == 0.0 || !finite_d(det)) return false;
    double u = det3(rhs, e2, c3) / det, v = det3(e1, rhs, c3) / det;
    const double r = det3(e1, e2, rhs) / det;
    if (!(finite_d(u) && finite_d(v) && finite_d(r))) return false;
    if (!(u >= -CELL_ACCEPT_TOL && v >= -CELL_ACCEPT_TOL && u + v <= 1.0 + CELL_ACCEPT_TOL && r > 0.0)) return false;
    u = u < 0.0 ? 0.0 : (u > 1.0 ? 1.0 : u);
    const double vmax = 1.0 - u;
    v = v < 0.0 ? 0.0 : (v > vmax ? vmax : v);
    w[0] = (1.0 - u) - v; w[1] = u; w[2] = v; w[3] = 0.0;
    return true;
}

// Bucket of a point of [-1, 1]^3 in the uniform nb^3 grid; the host's builder (functions.curvilinear_buckets) evaluates the
// same expression on the corners of every cell's enlarged box, and it is monotone in each coordinate.
__device__ __forceinline__ int bucket_coord(double x, int nb) {
    const int b = (int)((x + 1.0) * 0.5 * (double)nb);
    return b < 0 ? 0 : (b > nb - 1 ? nb - 1 : b);
}

// One target per thread.  Cells: quads j * ncx + i (ncx = nx when periodic: column i + 1 wraps and closes the seam, else
// nx - 1), then - periodic grids only - the cap triangles (pole, X[je, i], X[je, i+1]) of row 0 and of row ny - 1; the poles
// are the virtual nodes ny*nx and ny*nx + 1 whose unit vectors the host appends to X.  `bucket_cells` lists, ascending per
// bucket, every cell whose enlarged bounding box touches the bucket, so the first accepting candidate is the lowest
// accepting cell of all.  idx = -1: entry absent (never read); no accepting cell: four -1 and a count in *n_unmapped.
__global__ __launch_bounds__(BLOCK) void k_cell_locate(long long ntarg, const double *__restrict__ P, int ny, int nx, int periodic,
                                                       const double *__restrict__ X, int nb, const int *__restrict__ bucket_start,
                                                       const int *__restrict__ bucket_cells, int *__restrict__ idx,
                                                       double *__restrict__ w, unsigned int *__restrict__ n_unmapped) {
    const long long g = (long long)blockIdx.x * BLOCK + threadIdx.x;
    if (g >= ntarg) return;
    const Vec3 p = v3_load(P, g);
    int id[4] = {-1, -1, -1, -1};
    double wt[4] = {0.0, 0.0, 0.0, 0.0};
    bool found = false;
    if (p.x == p.x && p.y == p.y && p.z == p.z) {
        const int ncx = periodic ? nx : nx - 1, nq = (ny - 1) * ncx, nsrc = ny * nx;
        const long long b = ((long long)bucket_coord(p.x, nb) * nb + bucket_coord(p.y, nb)) * nb + bucket_coord(p.z, nb);
        const int k1 = bucket_start[b + 1];
        for (int k = bucket_start[b]; k < k1 && !found; ++k) {
            const int c = bucket_cells[k];
            if (c < 0 || c >= nq + (periodic ? 2 * nx : 0)) continue;      // not a cell: nothing is read for it
            if (c < nq) {
                const int j = c / ncx, i = c - j * ncx, ip = (i + 1 == nx) ? 0 : i + 1;
                const int a = j * nx + i, bb = j * nx + ip, cc = (j + 1) * nx + ip, d = (j + 1) * nx + i;
                if (cell_solve_quad(v3_load(X, a), v3_load(X, bb), v3_load(X, cc), v3_load(X, d), p, wt)) {
                    id[0] = a; id[1] = bb; id[2] = cc; id[3] = d; found = true;
                }
            } else {
                const int tri = c - nq, which = tri >= nx ? 1 : 0, i = tri - which * nx, ip = (i + 1 == nx) ? 0 : i + 1;
                const int row = which ? (ny - 1) * nx : 0;
                if (cell_solve_tri(v3_load(X, nsrc + which), v3_load(X, row + i), v3_load(X, row + ip), p, wt)) {
                    id[0] = nsrc + which; id[1] = row + i; id[2] = row + ip; id[3] = -1; found = true;
                }
            }
        }
    }
    if (!found) atomicAdd(n_unmapped, 1u);
#pragma unroll
    for (int k = 0; k < 4; ++k) { idx[4 * g + k] = id[k]; w[4 * g + k] = found ? wt[k] : 0.0; }
}

// Plain mean of the two edge rows of every plane, the value of the virtual pole nodes: (sum_i v[je, i]) / nx summed in index
// order, NaN propagating (a sibling of k_zonal_mean_rows, whose mean skips NaN and sums per lane).  One wave per
// (plane, row): 64 values per coalesced load, then every lane adds them in index order.
template <typename T>
__global__ __launch_bounds__(BLOCK) void k_row_mean_plain(long long nfield, int ny, int nx, const T *__restrict__ src,
                                                          double *__restrict__ pole /* [nfield][2] */) {
    const long long wv = ((long long)blockIdx.x * BLOCK + threadIdx.x) >> 6;
    const int lane = threadIdx.x & 63;
    if (wv >= nfield * 2) return;
    const long long f = wv >> 1;
    const int which = (int)(wv & 1);
    const T *r = src + (f * ny + (which ? ny - 1 : 0)) * (long long)nx;
    double sum = 0.0;
    for (int i0 = 0; i0 < nx; i0 += 64) {
        const double v = (i0 + lane < nx) ? (double)r[i0 + lane] : 0.0;
        const int n = nx - i0 < 64 ? nx - i0 : 64;
        for (int k = 0; k < n; ++k) sum = sum + __shfl(v, k, 64);
    }
    if (lane == 0) pole[f * 2 + which] = sum / (double)nx;
}

// Apply: out[f, g] = w0*v0, then + wk*vk for the present entries in order (values read in T, widened, stored in T); NaN in a
// present entry gives NaN; an unmapped target gets 0.0, or NaN with `unmapped_nan`.  Entries >= ny*nx are the pole values of
// k_row_mean_plain.  Write-dominated like k_regrid (1.9 of ~2.0 GB at production size), so: a thread owns W consecutive
// targets (16 bytes of a plane where the row length allows), keeps their idx / w in registers and walks the planes of its
// z-slice with streaming stores.  A block covers BLOCK * W consecutive targets; when the source elements they touch span at
// most SPARSE_WIN consecutive elements of a plane, the block stages that window per plane in LDS (coalesced loads, two
// buffers: one barrier per plane) and reads its entries from there instead of four uncoalesced gathers per output - what
// held the first k_regrid at 2.4 TB/s; a wider window (coarse, unsorted or seam-crossing targets) gathers directly.  Both
// forms read the same T values and do the same arithmetic: same bits.  `force_direct` is the test knob for the second form.
constexpr int SPARSE_WIN = 2048;

// The weighting rule of one target, the one copy k_regrid_sparse and k_regrid_sparse_wind share: w0*v0, then + wk*vk over
// the present entries in order; `value(k)` is only called for a present entry; no present entry: `miss`.
template <typename F>
__device__ __forceinline__ double sparse_weigh(const int (&id)[4], const double (&wt)[4], double miss, F &&value) {
    double acc = miss;
    bool have = false;
#pragma unroll
    for (int k = 0; k < 4; ++k)
        if (id[k] >= 0) {
            const double term = wt[k] * value(k);
            acc = have ? acc + term : term;
            have = true;
        }
    return acc;
}

template <typename T, int W>
__global__ __launch_bounds__(BLOCK) void k_regrid_sparse(long long nfield, long long nsrc, long long ntarg, unsigned int gz,
                                                         const T *__restrict__ src, const int *__restrict__ idx,
                                                         const double *__restrict__ w, const double *__restrict__ pole,
                                                         int unmapped_nan, int force_direct, T *__restrict__ out) {
    __shared__ T s_win[2][SPARSE_WIN];
    __shared__ int s_lo, s_hi;
    const long long g0 = ((long long)blockIdx.x * BLOCK + threadIdx.x) * W;
    const bool active = g0 < ntarg;                           // W | ntarg when W > 1: a thread's targets are all in range or none
    int id[W][4];
    double wt[W][4];
    if (threadIdx.x == 0) { s_lo = 0x7fffffff; s_hi = -1; }
    __syncthreads();
    int lo = 0x7fffffff, hi = -1;
#pragma unroll
    for (int u = 0; u < W; ++u)
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            id[u][k] = active ? idx[4 * (g0 + u) + k] : -1;
            if (id[u][k] >= nsrc + 2) id[u][k] = -1;           // nothing beyond the two pole nodes is ever read
            wt[u][k] = active ? w[4 * (g0 + u) + k] : 0.0;
            if (id[u][k] >= 0 && id[u][k] < nsrc) { lo = id[u][k] < lo ? id[u][k] : lo; hi = id[u][k] > hi ? id[u][k] : hi; }
        }
    if (hi >= 0) { atomicMin(&s_lo, lo); atomicMax(&s_hi, hi); }
    __syncthreads();
    const int w0 = s_lo, span = s_hi - s_lo + 1;              // span <= 0: the block reads no source element
    const bool staged = !force_direct && span > 0 && span <= SPARSE_WIN;
    const long long per = (nfield + gz - 1) / gz;
    const long long f0 = (long long)blockIdx.y * per, f1 = f0 + per < nfield ? f0 + per : nfield;
    const double miss = unmapped_nan ? __builtin_nan("") : 0.0;
    auto combine = [&](long long f, auto &&value) {
        double r[W];
#pragma unroll
        for (int u = 0; u < W; ++u)
            r[u] = sparse_weigh(id[u], wt[u], miss, [&](int k) {
                return id[u][k] >= nsrc ? pole[f * 2 + (id[u][k] - nsrc)] : value(id[u][k]);
            });
        if (active) storev_nt<T, W>(out + f * ntarg + g0, r);
    };
    if (staged) {
        int buf = 0;
        for (long long f = f0; f < f1; ++f, buf ^= 1) {
            const T *sp = src + f * nsrc + w0;
            for (int c = threadIdx.x; c < span; c += BLOCK) s_win[buf][c] = sp[c];
            __syncthreads();                                  // the other buffer is last read one plane back, before this barrier
            combine(f, [&](int i) { return (double)s_win[buf][i - w0]; });
        }
    } else {
        for (long long f = f0; f < f1; ++f) {
            const T *sp = src + f * nsrc;
            combine(f, [&](int i) { return (double)sp[i]; });
        }
    }
}

// ---- winds of a rotated-pole SOURCE grid (not in the reference): ua / va stored GRID-RELATIVE are turned to geographic with
// the source nodes' (cs, sn) - the inverse of rotate_uv's rotation: `sn` negated, k_rotate_pair's rule -, each component
// ROUNDED TO T, before they are weighted; each weighted value is ROUNDED TO T and, where the targets lie on a rotated grid
// too, the pair goes through rotate_uv with the target's (ct, st): the bits of pgw_rotate_pair(inverse), pgw_regrid_sparse on
// each component and pgw_rotate_pair.  A null cos / sin pair switches its rotation off (a uniform branch).

// k_row_mean_plain for the pair: the two edge-row means of the geographic, T-rounded components, summed in index order.
template <typename T>
__global__ __launch_bounds__(BLOCK) void k_row_mean_plain_wind(long long nfield, int ny, int nx, const T *__restrict__ src_u,
                                                               const T *__restrict__ src_v, const double *__restrict__ cs,
                                                               const double *__restrict__ sn, double *__restrict__ pole_u,
                                                               double *__restrict__ pole_v /* [nfield][2] each */) {
    const long long wv = ((long long)blockIdx.x * BLOCK + threadIdx.x) >> 6;
    const int lane = threadIdx.x & 63;
    if (wv >= nfield * 2) return;
    const long long f = wv >> 1;
    const int which = (int)(wv & 1);
    const long long row = (long long)(which ? ny - 1 : 0) * nx, at = f * ny * (long long)nx + row;
    double sum_u = 0.0, sum_v = 0.0;
    for (int i0 = 0; i0 < nx; i0 += 64) {
        T a = (T)0, b = (T)0;
        if (i0 + lane < nx) {
            a = src_u[at + i0 + lane];
            b = src_v[at + i0 + lane];
            if (cs) rotate_uv<T>((double)a, (double)b, cs[row + i0 + lane], -sn[row + i0 + lane], a, b);
        }
        const double u = (double)a, v = (double)b;
        const int n = nx - i0 < 64 ? nx - i0 : 64;
        for (int k = 0; k < n; ++k) { sum_u = sum_u + __shfl(u, k, 64); sum_v = sum_v + __shfl(v, k, 64); }
    }
    if (lane == 0) { pole_u[f * 2 + which] = sum_u / (double)nx; pole_v[f * 2 + which] = sum_v / (double)nx; }
}

// k_regrid_sparse on both components at once: a target's idx / w and its (ct, st) serve both.  The same two forms by the
// same rule, with a window of SPARSE_WIND_WIN elements: the staged form turns each source element of the window to
// geographic ONCE while it stages it (a thread stages the same SPARSE_WIND_WIN / BLOCK window elements of every plane and
// keeps their cs / sn in registers) and holds the T-rounded geographic pair in LDS, two buffers per component - at 1024
// elements that is 32 KiB of float64, what k_regrid_sparse holds, so as many blocks per CU; the direct form gathers a
// target's four pairs and their cs / sn (registers, once per z-slice) and turns them per target.  The host launches W = 2
// (or 1): four float32 targets per thread would need 310 registers for the entries' idx, w, cs and sn.
constexpr int SPARSE_WIND_WIN = 1024;

template <typename T, int W>
__global__ __launch_bounds__(BLOCK) void k_regrid_sparse_wind(long long nfield, long long nsrc, long long ntarg, unsigned int gz,
                                                              const T *__restrict__ src_u, const T *__restrict__ src_v,
                                                              const double *__restrict__ src_cos, const double *__restrict__ src_sin,
                                                              const int *__restrict__ idx, const double *__restrict__ w,
                                                              const double *__restrict__ pole_u, const double *__restrict__ pole_v,
                                                              int unmapped_nan, int force_direct,
                                                              const double *__restrict__ targ_cos, const double *__restrict__ targ_sin,
                                                              T *__restrict__ u_out, T *__restrict__ v_out) {
    constexpr int PER = SPARSE_WIND_WIN / BLOCK;              // window elements a thread stages per plane
    __shared__ T s_u[2][SPARSE_WIND_WIN], s_v[2][SPARSE_WIND_WIN];
    __shared__ int s_lo, s_hi;
    const long long g0 = ((long long)blockIdx.x * BLOCK + threadIdx.x) * W;
    const bool active = g0 < ntarg;                           // W | ntarg when W > 1, as k_regrid_sparse
    int id[W][4];
    double wt[W][4], ct[W], st[W];
    if (threadIdx.x == 0) { s_lo = 0x7fffffff; s_hi = -1; }
    __syncthreads();
    int lo = 0x7fffffff, hi = -1;
#pragma unroll
    for (int u = 0; u < W; ++u) {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            id[u][k] = active ? idx[4 * (g0 + u) + k] : -1;
            if (id[u][k] >= nsrc + 2) id[u][k] = -1;           // nothing beyond the two pole nodes is ever read
            wt[u][k] = active ? w[4 * (g0 + u) + k] : 0.0;
            if (id[u][k] >= 0 && id[u][k] < nsrc) { lo = id[u][k] < lo ? id[u][k] : lo; hi = id[u][k] > hi ? id[u][k] : hi; }
        }
        ct[u] = (targ_cos && active) ? targ_cos[g0 + u] : 1.0;
        st[u] = (targ_cos && active) ? targ_sin[g0 + u] : 0.0;
    }
    if (hi >= 0) { atomicMin(&s_lo, lo); atomicMax(&s_hi, hi); }
    __syncthreads();
    const int w0 = s_lo, span = s_hi - s_lo + 1;              // span <= 0: the block reads no source element
    const bool staged = !force_direct && span > 0 && span <= SPARSE_WIND_WIN;
    const long long per = (nfield + gz - 1) / gz;
    const long long f0 = (long long)blockIdx.y * per, f1 = f0 + per < nfield ? f0 + per : nfield;
    const double miss = unmapped_nan ? __builtin_nan("") : 0.0;
    // `pair(u, k, gu, gv)`: the geographic, T-rounded pair of a present entry that is a source element
    auto combine = [&](long long f, auto &&pair) {
        double ru[W], rv[W];
#pragma unroll
        for (int u = 0; u < W; ++u) {
            double gu[4], gv[4];
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (id[u][k] >= nsrc) { gu[k] = pole_u[f * 2 + (id[u][k] - nsrc)]; gv[k] = pole_v[f * 2 + (id[u][k] - nsrc)]; }
                else if (id[u][k] >= 0) pair(u, k, gu[k], gv[k]);
            T a = (T)sparse_weigh(id[u], wt[u], miss, [&](int k) { return gu[k]; });
            T b = (T)sparse_weigh(id[u], wt[u], miss, [&](int k) { return gv[k]; });
            if (targ_cos) rotate_uv<T>((double)a, (double)b, ct[u], st[u], a, b);
            ru[u] = (double)a; rv[u] = (double)b;
        }
        if (active) { storev_nt<T, W>(u_out + f * ntarg + g0, ru); storev_nt<T, W>(v_out + f * ntarg + g0, rv); }
    };
    if (staged) {
        double wc[PER], ws[PER];
#pragma unroll
        for (int j = 0; j < PER; ++j) {
            const int c = threadIdx.x + j * BLOCK;
            wc[j] = (src_cos && c < span) ? src_cos[w0 + c] : 1.0;
            ws[j] = (src_cos && c < span) ? -src_sin[w0 + c] : 0.0;
        }
        int buf = 0;
        for (long long f = f0; f < f1; ++f, buf ^= 1) {
            const T *pu = src_u + f * nsrc + w0, *pv = src_v + f * nsrc + w0;
#pragma unroll
            for (int j = 0; j < PER; ++j) {
                const int c = threadIdx.x + j * BLOCK;
                if (c < span) {
                    T a = pu[c], b = pv[c];
                    if (src_cos) rotate_uv<T>((double)a, (double)b, wc[j], ws[j], a, b);
                    s_u[buf][c] = a; s_v[buf][c] = b;
                }
            }
            __syncthreads();                                  // the other buffers are last read one plane back, before this barrier
            combine(f, [&](int u, int k, double &gu, double &gv) {
                gu = (double)s_u[buf][id[u][k] - w0]; gv = (double)s_v[buf][id[u][k] - w0];
            });
        }
    } else {
        double ec[W][4], es[W][4];
#pragma unroll
        for (int u = 0; u < W; ++u)
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const bool elem = src_cos && id[u][k] >= 0 && id[u][k] < nsrc;
                ec[u][k] = elem ? src_cos[id[u][k]] : 1.0;
                es[u][k] = elem ? -src_sin[id[u][k]] : 0.0;
            }
        for (long long f = f0; f < f1; ++f) {
            const T *pu = src_u + f * nsrc, *pv = src_v + f * nsrc;
            combine(f, [&](int u, int k, double &gu, double &gv) {
                T a = pu[id[u][k]], b = pv[id[u][k]];
                if (src_cos) rotate_uv<T>((double)a, (double)b, ec[u][k], es[u][k], a, b);
                gu = (double)a; gv = (double)b;
            });
        }
    }
}

}  // namespace pgw
