// pgw_device.h -- device-side helpers shared by the gfx950 kernels.
//
// Column kernels: one thread owns V adjacent (lat,lon) columns (V*sizeof(T) = 16 B where the
// grid allows it), consecutive lanes own consecutive groups, so every level access of a wave is
// one fully coalesced 1 KiB row segment of the (time, lev, lat, lon) C-order array.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <type_traits>
#include "pgw_log_table.h"

namespace pgw {

constexpr double CON_RD = 287.05;      // constants.py:3-7 of the reference
constexpr double CON_G = 9.80665;
constexpr double CON_MW_MD = 0.622;

constexpr int BLOCK = 256;             // 4 waves of 64

// device-resident status block of a context (zeroed before a launch that can report)
struct DevStatus {
    int code;                          // first pgw_status reported by a kernel (10: one of 10 .. 12, see report_ordered)
    int nan_seen;                      // bit 0: NaN in target min, bit 1: NaN in source min
    unsigned long long col;            // min offending column (init ~0ull); codes 10 .. 12: min of (column << 2 | code - 10)
    unsigned long long max_bits;       // max |err| as ordered bits of a non-negative double
    unsigned long long valid;          // number of non-NaN |err| contributions (>0 flag)
    unsigned long long min_targ_bits;  // min target pressure (bits of positive double)
    unsigned long long min_src_bits;   // min source pressure
    unsigned long long levels_touched; // sum over columns of levels read (early-exit kernels)
    unsigned long long qv_stored;      // sum over columns of levels whose QV the pass stored (k_ps_loop_multi, last pass of a launch)
};

template <typename T, int V> struct alignas(sizeof(T) * V) Pack { T v[V]; };

template <typename T, int V>
__device__ __forceinline__ void loadv(const T *__restrict__ p, double (&out)[V]) {
    Pack<T, V> t = *reinterpret_cast<const Pack<T, V> *>(p);
#pragma unroll
    for (int i = 0; i < V; ++i) out[i] = (double)t.v[i];
}

template <typename T, int V>
__device__ __forceinline__ void storev(T *__restrict__ p, const double (&in)[V]) {
    Pack<T, V> t;
#pragma unroll
    for (int i = 0; i < V; ++i) t.v[i] = (T)in[i];
    *reinterpret_cast<Pack<T, V> *>(p) = t;
}

// streaming (non-temporal) forms of loadv / storev, see ld_off_nt below
template <typename T, int V> struct VecOf { typedef T type __attribute__((ext_vector_type(V))); };
template <typename T, int V>
__device__ __forceinline__ void loadv_nt(const T *__restrict__ p, double (&out)[V]) {
    if constexpr (V == 1) out[0] = (double)__builtin_nontemporal_load(p);
    else if constexpr (sizeof(T) * V > 16) {          // a row wider than one access (double beside float32 rows): 16-byte pieces
        constexpr int H = 16 / sizeof(T);
#pragma unroll
        for (int h = 0; h < V; h += H) {
            typename VecOf<T, H>::type t = __builtin_nontemporal_load(reinterpret_cast<const typename VecOf<T, H>::type *>(p + h));
#pragma unroll
            for (int i = 0; i < H; ++i) out[h + i] = (double)t[i];
        }
    } else {
        typename VecOf<T, V>::type t = __builtin_nontemporal_load(reinterpret_cast<const typename VecOf<T, V>::type *>(p));
#pragma unroll
        for (int i = 0; i < V; ++i) out[i] = (double)t[i];
    }
}
template <typename T, int V>
__device__ __forceinline__ void storev_nt(T *__restrict__ p, const double (&in)[V]) {
    if constexpr (V == 1) __builtin_nontemporal_store((T)in[0], p);
    else {
        typename VecOf<T, V>::type t;
#pragma unroll
        for (int i = 0; i < V; ++i) t[i] = (T)in[i];
        __builtin_nontemporal_store(t, reinterpret_cast<typename VecOf<T, V>::type *>(p));
    }
}

// loadv / storev for kernels whose operands differ in element size: at most 16 bytes per access (V float64 elements are
// V / 2 accesses), the single access of loadv / storev otherwise
template <typename T, int V>
__device__ __forceinline__ void loadv16(const T *__restrict__ p, double (&out)[V]) {
    if constexpr (sizeof(T) * V <= 16) loadv<T, V>(p, out);
    else {
        constexpr int H = 16 / sizeof(T);
#pragma unroll
        for (int h = 0; h < V; h += H) {
            Pack<T, H> t = *reinterpret_cast<const Pack<T, H> *>(p + h);
#pragma unroll
            for (int i = 0; i < H; ++i) out[h + i] = (double)t.v[i];
        }
    }
}
template <typename T, int V>
__device__ __forceinline__ void storev16(T *__restrict__ p, const double (&in)[V]) {
    if constexpr (sizeof(T) * V <= 16) storev<T, V>(p, in);
    else {
        constexpr int H = 16 / sizeof(T);
#pragma unroll
        for (int h = 0; h < V; h += H) {
            Pack<T, H> t;
#pragma unroll
            for (int i = 0; i < H; ++i) t.v[i] = (T)in[h + i];
            *reinterpret_cast<Pack<T, H> *>(p + h) = t;
        }
    }
}

// ---- addressing with 32-bit byte offsets ---------------------------------------------------
// `base + (long long)index` makes the compiler carry a 64-bit address per array and lane (two VGPRs and a 64-bit
// add per access).  When a whole array is smaller than 4 GiB the element can be addressed as uniform base (SGPR
// pair) + 32-bit byte offset in one VGPR, which is the form global_load / global_store take natively (saddr +
// voffset): one offset register serves every array of the same shape.  O is the offset type: unsigned int for
// that form, unsigned long long for arrays of 4 GiB and more.
using boff32 = unsigned int;          // byte offset types for ld_off / st_off
using boff64 = unsigned long long;
template <typename T, typename O>
__device__ __forceinline__ T ld_off(const T *__restrict__ base, O byte_off) {
    return *reinterpret_cast<const T *>(reinterpret_cast<const char *>(base) + byte_off);
}
template <typename T, typename O>
__device__ __forceinline__ void st_off(T *__restrict__ base, O byte_off, T v) {
    *reinterpret_cast<T *>(reinterpret_cast<char *>(base) + byte_off) = v;
}

// Streaming forms (the `nt` bit of global_load / global_store): data that is touched once per launch - the ERA fields in,
// the PGW fields out - should not displace what IS re-read (delta records, the loop's rows) from L2 / Infinity Cache, and a
// mixed read + write stream runs ~10 % faster with them (tools/micro/chunk_pattern.hip: 5.0 -> 5.6 TB/s at 128 threads).
template <typename T, typename O>
__device__ __forceinline__ T ld_off_nt(const T *__restrict__ base, O byte_off) {
    return __builtin_nontemporal_load(reinterpret_cast<const T *>(reinterpret_cast<const char *>(base) + byte_off));
}
template <typename T, typename O>
__device__ __forceinline__ void st_off_nt(T *__restrict__ base, O byte_off, T v) {
    __builtin_nontemporal_store(v, reinterpret_cast<T *>(reinterpret_cast<char *>(base) + byte_off));
}

// first reported code wins (kernels of a stream run in order, so an earlier kernel's error outlives later ones);
// the column is the smallest one that reported THAT code
__device__ __forceinline__ void report(DevStatus *st, int code, long long col) {
    int prev = atomicCAS(&st->code, 0, code);
    if (prev == 0 || prev == code) atomicMin(&st->col, (unsigned long long)col);
}

// The three errors of the reference's column loop (functions.py:493-508, 564-566) - 10 source ends, 11 target ends, 12 a target
// out of range in 'off' mode: the reference walks the columns in (time, lat, lon) order and makes the checks in that
// order within a column, so the call raises what the SMALLEST flat column holds, and the smallest code of that column.
// `code` becomes ORDERED_CODE_FIRST as the mark of such a status and `col` the minimum of (column << 2 | code - 10) over
// every report; `ordered_status` takes the pair apart on the host.  Like `report`, only for a status no other code is in.
constexpr int ORDERED_CODE_FIRST = 10;
__device__ __forceinline__ void report_ordered(DevStatus *st, int code, long long col) {
    int prev = atomicCAS(&st->code, 0, ORDERED_CODE_FIRST);
    if (prev == 0 || prev == ORDERED_CODE_FIRST)
        atomicMin(&st->col, ((unsigned long long)col << 2) | (unsigned long long)(code - ORDERED_CODE_FIRST));
}
// code and column of a fetched status (host side)
inline void ordered_status(const DevStatus &st, int *code, long long *col) {
    *code = st.code; *col = (long long)st.col;
    if (st.code == ORDERED_CODE_FIRST) {
        *code = ORDERED_CODE_FIRST + (int)(st.col & 3ull);
        *col = (long long)(st.col >> 2);
    }
}

// ---- division by a value that many numerators share ---------------------------------------
// The compiler expands an IEEE fp64 division into v_div_scale x2, v_rcp, two Newton steps on the reciprocal,
// q = n*r, one residual correction (v_div_fmas) and v_div_fixup: 11 instructions.  When many numerators are
// divided by the same d, the reciprocal part (v_rcp + 4 FMAs) is computed once and each quotient costs the last
// three instructions.  The arithmetic is the compiler's own sequence, so quotients are bit-identical whenever
// v_div_scale would not rescale (finite operands whose exponents are far from the denormal / overflow range -
// true for every divisor this is used with: grid spacings and ln-pressure intervals); NaN numerators propagate,
// a -0 numerator gives +0 (v_div_fixup would restore the sign; the value is the same).
// Not for divisors that can be 0, infinite or denormal-scale.
struct SharedDivisor {
    double d, r;
    __device__ __forceinline__ explicit SharedDivisor(double den) : d(den) {
        double y = __builtin_amdgcn_rcp(den);
        y = __builtin_fma(__builtin_fma(-den, y, 1.0), y, y);
        y = __builtin_fma(__builtin_fma(-den, y, 1.0), y, y);
        r = y;
    }
    // divisor known at compile time: r must be the double nearest to 1/den (then the quotient below is the
    // correctly rounded one - Markstein's theorem - and therefore the same bits as any IEEE division)
    __device__ __forceinline__ constexpr SharedDivisor(double den, double rcp_nearest) : d(den), r(rcp_nearest) {}
    __device__ __forceinline__ double divide(double n) const {
        double q = n * r;
        return __builtin_fma(__builtin_fma(-d, q, n), r, q);
    }
};

// n / d by the same steps for a divisor used once: the compiler's IEEE fp64 division without v_div_scale (x2) and
// v_div_fixup - 8 instead of 11 instructions, the correctly rounded quotient (the same bits) whenever neither operand
// needs scaling and d is finite and non-zero; used where the divisor is a physical quantity of known range
// (a temperature offset, a pressure minus a vapour-pressure fraction, 0.622 + 0.378 q, e_sat).  NaN operands give
// NaN like the division; d = 0 or inf gives NaN where the division gives inf / 0.
__device__ __forceinline__ double div_ns(double n, double d) { return SharedDivisor(d).divide(n); }

// ---- natural logarithm ------------------------------------------------------------------
// Every kernel on the path takes one ln(p) per level and column, and with fp64 vector math at
// half rate the generic ocml log (~65 instructions, double-double internals, denormal /
// negative / inf handling) made the column kernels VALU-bound.  pgw_log is the classic
// fdlibm __ieee754_log kernel (argument reduction to [sqrt(1/2), sqrt(2)), s = f/(2+f),
// degree-14 even polynomial; documented error < 1 ulp) for positive normal finite x, with the
// quotient formed by v_rcp_f64 + two Newton steps + one residual correction; everything else
// (0, negative, denormal, inf, NaN) goes to the ocml log.  One implementation serves table
// entries and per-column values, so `src_x == targ_x` comparisons (functions.py:540) are
// consistent.  Against the exact logarithm (tests/test_device_math_hip.py::test_log_true_error_is_at_most_one_ulp,
// 111 000 arguments from bit patterns: every interval end of the table below in 12 binades, the arguments whose logarithm
// lies just under a power of two, the neighbourhood of 1): at most 0.758 ulp; the test requires <= 1.
// keeps a rarely taken block a real (wave-uniform) branch: volatile asm cannot be speculated, so
// the compiler does not if-convert the block into "compute both sides and select"
__device__ __forceinline__ double no_speculate(double x) {
    asm volatile("" : "+v"(x));
    return x;
}

// one Horner step a*b + c as the three-address v_fma_f64, c (a coefficient that stays live) in its own register
__device__ __forceinline__ double fma3(double a, double b, double c) {
#ifdef PGW_NO_FMA3
    return __builtin_fma(a, b, c);
#else
    double d;
#ifdef PGW_FMA3_SGPR
    // A/B knob: the coefficient in a scalar register pair (the one constant-bus operand a VOP3 instruction may take) - no
    // vector register is held for it, s_mov_b32 literals on the scalar unit materialise it.  Every file-path kernel then
    // compiles without scratch (k_delta_quad<float, double, REF>: 127 VGPRs / 0 B instead of 128 / 180 B; k_reinterp_pair
    // with e: 139 / 0 instead of 168 / 116) and runs in the same time (round 3, same box: 2.13 / 2.14, 1.61 / 1.60,
    // 1.594 / 1.596 ms) - the spilled values are constants of cold paths.  Not the default.
    asm("v_fma_f64 %0, %1, %2, %3" : "=v"(d) : "v"(a), "v"(b), "s"(c));
#else
    asm("v_fma_f64 %0, %1, %2, %3" : "=v"(d) : "v"(a), "v"(b), "v"(c));
#endif
    return d;
#endif
}
// F3: Horner steps as three-address FMAs (fma3) - for kernels whose register budget is not the binding one
template <bool F3, bool CHECK = true>
__device__ __forceinline__ double pgw_log_impl(double x) {
    if (CHECK && __builtin_expect(!(x >= 2.2250738585072014e-308 && x <= 1.7976931348623157e308), 0))
        return log(no_speculate(x));
    const double ln2_hi = 6.93147180369123816490e-01, ln2_lo = 1.90821492927058770002e-10;
    const double Lg1 = 6.666666666666735130e-01, Lg2 = 3.999999999940941908e-01, Lg3 = 2.857142874366239149e-01,
                 Lg4 = 2.222219843214978396e-01, Lg5 = 1.818357216161805012e-01, Lg6 = 1.531383769920937332e-01,
                 Lg7 = 1.479819860511658591e-01;
    int k = __builtin_amdgcn_frexp_exp(x);                 // x = m * 2^k, m in [0.5, 1)
    double m = __builtin_amdgcn_frexp_mant(x);
    if (m < 0.70710678118654752440) { m = m * 2.0; k -= 1; }
    double f = m - 1.0;                                    // exact
    double d = 2.0 + f;                                    // in [1.70, 2.42)
    double r = __builtin_amdgcn_rcp(d);
    r = __builtin_fma(__builtin_fma(-d, r, 1.0), r, r);
    r = __builtin_fma(__builtin_fma(-d, r, 1.0), r, r);
    double s = f * r;
    s = __builtin_fma(__builtin_fma(-d, s, f), r, s);      // s = f / (2 + f), correctly rounded up to ~0.5 ulp
    double dk = (double)k;
    double z = s * s;
    double w = z * z;
    double t1, t2;
    if (F3) {
        t1 = w * fma3(w, fma3(w, Lg6, Lg4), Lg2);
        t2 = z * fma3(w, fma3(w, fma3(w, Lg7, Lg5), Lg3), Lg1);
    } else {
        t1 = w * __builtin_fma(w, __builtin_fma(w, Lg6, Lg4), Lg2);
        t2 = z * __builtin_fma(w, __builtin_fma(w, __builtin_fma(w, Lg7, Lg5), Lg3), Lg1);
    }
    double R = t2 + t1;
    double hfsq = 0.5 * f * f;
    return dk * ln2_hi - ((hfsq - __builtin_fma(s, hfsq + R, dk * ln2_lo)) - f);
}
__device__ __forceinline__ double pgw_log(double x) { return pgw_log_impl<false>(x); }
__device__ __forceinline__ double pgw_log_f3(double x) { return pgw_log_impl<true>(x); }    // same bits

// The fdlibm kernel again, with the quotient s = f / (2 + f) and the final sum k ln2 + f - f^2/2 + s (f^2/2 + R) carried as
// double-double pairs (error-free two-sums, FMA residuals): at most 0.513 ulp from the exact logarithm on every argument tried
// (the test requires <= 0.55), and the correctly rounded double for all but 2.3 in 10^4 of the pressures of the path (uniform in
// 1e-4 .. 1.1e5 Pa; required: <= 1 in 10^3) - elsewhere the share differs: 0.5 in 10^4 over all magnitudes, 8.5 in 10^4 on the
// interval ends of the table below, 15 in 10^4 where ln x lies just under a power of two
// (tests/test_device_math_hip.py::test_log_dd_true_error_and_share_correctly_rounded, exact reference).  pgw_log is not the
// correctly rounded double for 1.1 % of those pressures and 2.9 % of the interval ends.  About twice the
// instructions: for the few logarithms whose last bit reaches a float64 RESULT - the final expression of integ_geopot
// (functions.py:174-179) in the reference's dtype flow, which is compared with numpy's bit for bit - not for level loops.
__device__ __forceinline__ void two_sum(double a, double b, double &s, double &e) {
    s = a + b;
    const double bb = s - a;
    e = (a - (s - bb)) + (b - bb);
}
__device__ __forceinline__ double pgw_log_dd(double x) {
    if (__builtin_expect(!(x >= 2.2250738585072014e-308 && x <= 1.7976931348623157e308), 0)) return log(no_speculate(x));
    const double ln2_hi = 6.93147180369123816490e-01, ln2_lo = 1.90821492927058770002e-10;
    const double Lg1 = 6.666666666666735130e-01, Lg2 = 3.999999999940941908e-01, Lg3 = 2.857142874366239149e-01,
                 Lg4 = 2.222219843214978396e-01, Lg5 = 1.818357216161805012e-01, Lg6 = 1.531383769920937332e-01,
                 Lg7 = 1.479819860511658591e-01;
    int k = __builtin_amdgcn_frexp_exp(x);
    double m = __builtin_amdgcn_frexp_mant(x);
    if (m < 0.70710678118654752440) { m = m * 2.0; k -= 1; }
    const double f = m - 1.0;                              // exact
    const double d_hi = 2.0 + f, d_lo = f - (d_hi - 2.0);  // 2 + f as a pair (|f| < 2: fast two-sum)
    double r = __builtin_amdgcn_rcp(d_hi);
    r = __builtin_fma(__builtin_fma(-d_hi, r, 1.0), r, r);
    r = __builtin_fma(__builtin_fma(-d_hi, r, 1.0), r, r);
    double s = f * r;
    s = __builtin_fma(__builtin_fma(-d_hi, s, f) - d_lo * s, r, s);
    const double s_lo = (__builtin_fma(-d_hi, s, f) - d_lo * s) * r;
    const double dk = (double)k, z = s * s, w = z * z;
    const double t1 = w * __builtin_fma(w, __builtin_fma(w, Lg6, Lg4), Lg2);
    const double t2 = z * __builtin_fma(w, __builtin_fma(w, __builtin_fma(w, Lg7, Lg5), Lg3), Lg1);
    const double R = t2 + t1 + 2.0 * s * s_lo * Lg1;       // first-order effect of s_lo on z = s^2
    const double hf = 0.5 * f, h_hi = hf * f, h_lo = __builtin_fma(hf, f, -h_hi);
    double u_hi, u_lo;
    two_sum(h_hi, R, u_hi, u_lo);
    u_lo += h_lo;
    const double T_hi = s * u_hi, T_lo = __builtin_fma(s, u_hi, -T_hi) + s * u_lo + s_lo * u_hi;
    double a_hi, a_lo, e;
    two_sum(dk * ln2_hi, f, a_hi, a_lo);                   // k ln2_hi is exact (21 trailing zero bits)
    two_sum(a_hi, -h_hi, a_hi, e); a_lo += e;
    two_sum(a_hi, T_hi, a_hi, e); a_lo += e;
    a_lo += (T_lo - h_lo) + dk * ln2_lo;
    return a_hi + a_lo;
}

// ---- table-driven natural logarithm for the level loops ------------------------------------
// The level loops of the surface-pressure iteration are bound by fp64 issue (94 % of the SIMD cycles), and the
// fdlibm kernel above is ~40 of their ~90 instructions per level.  Tang-style table method (the construction of
// glibc's / ARM optimized-routines' log): x = 2^k z, z in [0.6875, 1.375) cut into 128 intervals by the top mantissa
// bits; per interval a double invc ~ 1/centre and logc = -log(invc), the pair chosen (tools/gen_log_table.py) such that
// logc is within 2.2e-19 of the exact value; r = fma(z, invc, -1) (|r| < 0.0040, one rounding), and
//     log x = (k ln2_hi + logc) + r + [r^2 (A0 + A1 r + ... + A5 r^5) + k ln2_lo]     (truncation r^8/8 < 1e-20)
// with the leading sum split exactly into hi + lo.  ~25 instructions and one 16-B LDS read.  The two intervals next to
// z = 1 with k = 0 (results near zero, where the table's absolute accuracy is not a relative one) and everything
// outside the positive normal range go to pgw_log.
// Accuracy: NOT within 1 ulp of the exact logarithm.  w = fma(k, ln2_hi, logc) is rounded once and that rounding is not
// compensated (lo compensates only h = w + r); where the result lies one binade below w - ln x just under 1/2, 1, 2, 4, 8:
// x just under sqrt(e), e, e^2, e^4, e^8 = 2981 Pa - half an ulp of w is a whole ulp of the result.  Bound: 0.5 (final
// rounding) + 1.0 (w) + 0.25 (logc's 2.2e-19 against the smallest result ulp 2^-60) + 0.05 (the rest) = 1.8 ulp; the result
// cannot lie two binades below a rounded w (for k = 0, w = logc is exact; otherwise |w| >= ln 1.375 = 0.318 and |r| < 0.004).
// Measured maximum: 1.489 ulp at x = 1.6487212707001178 (the double below sqrt(e); 1.334 at x = 1.6484375); above 1 ulp only
// under sqrt(e) among 111 000 arguments; up to a quarter of the results (25 % of the pressures of the path, 0.2 % over all
// magnitudes) are not the correctly rounded double.  1e-16
// relative: harmless to the physics, and the distance to numpy's log (itself up to 0.52 ulp off) stays <= 1 ulp
// (tests/test_hip_parity.py::test_device_log_accuracy).  Established by an exact restatement of the function in
// tests/device_math_cases.py, held to the exact logarithm and the 1.8 ulp on the CPU (tests/test_device_math_host.py, which
// also checks the table's two bounds quoted above) and equal to this function bit for bit on the GPU
// (tests/test_device_math_hip.py::test_log_tab_is_its_restatement_bit_for_bit).
// The table lives in LDS (stage_log_table): lanes index it with their own interval.
__device__ const double LOG_TABLE_DEV[2 * LOG_TABLE_N] = {
#define PGW_LOG_TABLE_BODY
#include "pgw_log_table.h"
#undef PGW_LOG_TABLE_BODY
};
__device__ __forceinline__ void stage_log_table(double *lds, int nthreads) {      // caller synchronises afterwards
    for (int i = threadIdx.x; i < 2 * LOG_TABLE_N; i += nthreads) lds[i] = LOG_TABLE_DEV[i];
}
__device__ __forceinline__ double pgw_log_tab(double x, const double *tab) {
    const unsigned int hi = (unsigned int)__double2hiint(x);
    const unsigned int thi = hi - 0x3FE60000u;                      // (bits(x) - OFF) >> 32; OFF's low word is 0: no borrow
    // positive normal finite x  <=>  0x00100000 <= hi < 0x7FF00000
    const int i = (int)((thi >> 13) & 127u);
    const int k = (int)thi >> 20;
    // one divergent region for both exceptions: not a positive normal finite number (library log), or within two table
    // intervals of 1, where r = z/c - 1 cancels (fdlibm kernel; pgw_log_impl sends non-normal arguments to the library itself)
    if (__builtin_expect(!(hi - 0x00100000u < 0x7FE00000u) || (k == 0 && (i == 79 || i == 80)), 0))
        return pgw_log_impl<true, true>(no_speculate(x));
    const double z = __hiloint2double((int)(hi - (thi & 0xFFF00000u)), __double2loint(x));
    const double invc = tab[2 * i], logc = tab[2 * i + 1];
    const double r = __builtin_fma(z, invc, -1.0);
    const double kd = (double)k;
    const double w = __builtin_fma(kd, 0x1.62e42fefa3800p-1, logc);       // k ln2_hi is exact (11 trailing zero bits)
    const double h = w + r;
    const double lo = __builtin_fma(kd, 0x1.ef35793c76730p-45, (w - h) + r);
    const double r2 = r * r;
    double p = fma3(r, 0x1.2492492492492p-3, -0x1.5555555555555p-3);       //  1/7, -1/6
    p = fma3(r, p, 0x1.999999999999ap-3);                                   //  1/5
    p = fma3(r, p, -0x1.0p-2);                                              // -1/4
    p = fma3(r, p, 0x1.5555555555555p-2);                                   //  1/3
    p = fma3(r, p, -0x1.0p-1);                                              // -1/2
    return __builtin_fma(r2, p, lo) + h;
}

// ---- exponential --------------------------------------------------------------------------
// The same arithmetic as the device library's exp(double) - n = rint(x log2 e), r = x - n ln2 (two FMAs),
// degree-11 polynomial in r (Horner), ldexp, the library's two range selects - written out with explicit FMAs.
// Same operations and constants, hence the same bits as exp() (tests/...::test_device_exp_is_library_exp); the point
// is code generation: for most of the inlined library instances in the delta kernels the compiler forms each Horner
// step as v_mov_b64 (copy of the coefficient) + v_fmac, two instructions, where one three-address v_fma_f64 does.
template <bool RANGE, bool GUARD = false>
__device__ __forceinline__ double pgw_exp_impl(double x) {
    const double n = __builtin_rint(x * 0x1.71547652b82fep+0);
    double r = __builtin_fma(-0x1.62e42fefa39efp-1, n, x);
    r = __builtin_fma(-0x1.abc9e3b39803fp-56, n, r);
    if (GUARD) {
        // beyond |x| ~ 2^50 the product x log2(e) is not exact to a unit, n is off by many and r is not a reduced remainder:
        // the polynomial's value, and with it the sign of the saturated ldexp, would be arbitrary (-0 / -inf were measured
        // from |x| = 1.4e17).  The result is decided by n alone from |x| = 1076 on, so r = x - x there: 0 for a finite x
        // (p = 1 exactly), NaN for +-inf; a NaN x compares false and keeps its NaN r.  Same bits for every |x| <= 2000.
        const double z = x - x;
        r = (__builtin_fabs(x) > 2000.0) ? z : r;
    }
    double p = fma3(0x1.ade156a5dcb37p-26, r, 0x1.28af3fca7ab0cp-22);
    p = fma3(r, p, 0x1.71dee623fde64p-19);
    p = fma3(r, p, 0x1.a01997c89e6b0p-16);
    p = fma3(r, p, 0x1.a01a014761f6ep-13);
    p = fma3(r, p, 0x1.6c16c1852b7b0p-10);
    p = fma3(r, p, 0x1.1111111122322p-7);
    p = fma3(r, p, 0x1.55555555502a1p-5);
    p = fma3(r, p, 0x1.5555555555511p-3);
    p = fma3(r, p, 0x1.000000000000bp-1);
    p = __builtin_fma(r, p, 1.0);
    p = __builtin_fma(r, p, 1.0);
    double v = __builtin_ldexp(p, (int)n);
    if (RANGE) {
        v = (1024.0 < x) ? __builtin_inf() : v;      // NaN compares false: the NaN from the arithmetic is kept
        v = (x < -1075.0) ? 0.0 : v;
    }
    return v;
}
__device__ __forceinline__ double pgw_exp(double x) { return pgw_exp_impl<true>(x); }
// Three forms of one arithmetic.  pgw_exp: the library's, with its two range selects (six instructions).
// pgw_exp_reduced: neither selects nor guard, for callers that use the value only where |x| <= 1000 and replace it elsewhere -
// the same bits as pgw_exp there (tests/test_device_math_hip.py::test_exp_reduced_is_exp_on_its_range); beyond |x| ~ 2^50 the
// sign of the saturated result is arbitrary.  It is what the kernels call: e_sat's one unconditional exponential (esat_mixed,
// |x| < 130 wherever the value is kept; tests/...::test_esat_fast_path_is_the_literal_expression goes through every temperature
// at which it is replaced, the zero divisors with |x| up to 5.6e19 included) and the Magnus formula of step_01 (|x| < 700).
// pgw_exp_finite: no selects but the guard on r above (four instructions), the same bits as pgw_exp for EVERY finite x and for
// NaN - v_ldexp_f64 saturates to 0 / inf by itself, the conversion of n saturates too, and r is a reduced remainder or zero, so
// the polynomial is positive and finite; only x = +-inf gives NaN instead of inf / 0
// (tests/...::test_exp_finite_is_exp_for_every_finite_argument).  No kernel calls it at present - the guard in the delta
// kernels cost 0.15 % of a file for a value esat_mixed throws away; it is the form for an argument that is finite but not bounded.
__device__ __forceinline__ double pgw_exp_finite(double x) { return pgw_exp_impl<false, true>(x); }
__device__ __forceinline__ double pgw_exp_reduced(double x) { return pgw_exp_impl<false, false>(x); }

// ---- humidity thermodynamics (functions.py:58-125), operation order as written there ----
__device__ __forceinline__ double esat_water(double ta) {   // :74-89 water
    return 611.21 * pgw_exp(div_ns(17.502 * (ta - 273.16), ta - 32.19));
}
__device__ __forceinline__ double esat_ice(double ta) {     // :74-89 ice (a4 = -0.7)
    return 611.21 * pgw_exp(22.587 * (ta - 273.16) / (ta - (-0.7)));
}
// :91-105.  alpha = 1 (T>=T0), 0 (T<=Ti), ((T-Ti)/(T0-Ti))^2 in between, NaN for NaN T.
// alpha*e_w + (1-alpha)*e_i is evaluated in full only in the mixed range; for alpha in {0,1}
// the dropped term is exactly 0*finite = 0, so the value is unchanged: e_w and e_i are finite for
// 32.19 K < T <= 1e300 (tests/test_device_math_hip.py::test_esat_fast_path_is_the_literal_expression: the
// reference's expression bit for bit at every limit below, +-inf and NaN included).  Not for finite T
// between 7.96e306 and 1.03e307: there a3 (T - T0) overflows, the literal expression is 0 * inf = NaN
// and this one is finite.  Known; no branch is spent on it.
// One unconditional division + exp evaluates the phase every temperature needs (water for
// T >= T0, ice otherwise; the coefficients are selected, not the results), and only lanes in the
// mixed range take a real branch (no_speculate) for the second one.
// the temperatures the one-exponential value does not serve: mixed phase, unphysically cold, NaN
__device__ __forceinline__ double esat_special(double ta, double e1) {
    const double T0 = 273.16, Ti = 250.16;
    if (ta < T0 && ta > Ti) {                                    // mixed phase
        double ew = esat_water(ta);
        // (ta - Ti) / (T0 - Ti): T0 - Ti = 273.16 - 250.16 = 0x1.7000000000008p+4 in double (not 23); with the double nearest to
        // its reciprocal the two-step quotient is the correctly rounded one (Markstein), i.e. the bits of the division
        static_assert(273.16 - 250.16 == 0x1.7000000000008p+4, "T0 - Ti");
        double r = SharedDivisor(0x1.7000000000008p+4, 0x1.642c8590b215cp-5).divide(ta - Ti);
        double alpha = r * r;                                    // np.power(x, 2.) == x*x
        return alpha * ew + (1 - alpha) * e1;
    }
    if (ta <= 40.0) {                                            // unphysical cold: the literal expression, 0 * e_w may be NaN / inf
        const double ew = 611.21 * pgw_exp(17.502 * (ta - 273.16) / (ta - 32.19));     // IEEE division: the divisor is 0 at 32.19 K
        const double ei = 611.21 * pgw_exp(22.587 * (ta - 273.16) / (ta - (-0.7)));    // and at -0.7 K: exp(-inf) = 0
        return 0.0 * ew + 1.0 * ei;
    }
    return __builtin_nan("");                                    // NaN temperature
}
__device__ __forceinline__ double esat_mixed(double ta) {
    const double T0 = 273.16, Ti = 250.16;
    const bool warm = (ta >= T0);
    const double a3 = warm ? 17.502 : 22.587;
    const double a4 = warm ? 32.19 : -0.7;
    // e_w if warm else e_i (NaN for NaN ta); |argument| < 130 for every T the value is used for: no range selects
    double e1 = 611.21 * pgw_exp_reduced(div_ns(a3 * (ta - T0), ta - a4));
    // ONE divergent region per call (every branch costs scalar instructions and issue slots the few resident waves of the
    // delta kernels cannot hide): e1 is the answer for T >= T0 and for 40 K < T <= Ti
    if (__builtin_expect(!(warm || (ta <= Ti && ta > 40.0)), 0)) e1 = esat_special(no_speculate(ta), e1);
    return e1;
}
// div_ns followed by the division's own last instruction, v_div_fixup: the sign of a zero quotient (div_ns turns a -0
// numerator into +0) and the IEEE results for zero and infinite operands come back, finite non-zero quotients pass through
// unchanged.  For q -> RH, whose value for q = -0.0 numpy gives as -0.0
// (tests/test_device_math_hip.py::test_specific_to_relative_humidity_is_the_numpy_expression).
__device__ __forceinline__ double div_ns_fixup(double n, double d) { return __builtin_amdgcn_div_fixup(div_ns(n, d), d, n); }
__device__ __forceinline__ double q_to_e(double hus, double pa) {          // :58-64
    return div_ns_fixup(hus * pa, CON_MW_MD + 0.378 * hus);
}
__device__ __forceinline__ double e_to_q(double vapp, double pa) {         // :66-72
    return CON_MW_MD * vapp / (pa - (1 - CON_MW_MD) * vapp);
}
// the same with the scale-free quotient, for pressures of the model's levels (pa - 0.378 e is a pressure of known range)
__device__ __forceinline__ double e_to_q_ns(double vapp, double pa) {
    return div_ns(CON_MW_MD * vapp, pa - (1 - CON_MW_MD) * vapp);
}
__device__ __forceinline__ double q_to_rh(double hus, double pa, double ta) {   // :107-116
    return div_ns_fixup(q_to_e(hus, pa), esat_mixed(ta)) * 100;
}
// ---- reference-dtype mode: RELHUM of a float32 ERA state as numpy's promotion evaluates functions.py:58-116 ----
// e_sat of a float32 temperature is float32 throughout (alpha = full_like(ta): :95-98; a1*np.exp(a3*(ta-T0)/(ta-a4)):
// :88 with the python floats taken as float32 scalars); every operation below is one IEEE float32 operation except
// expf (<= 1 ulp here; numpy's SIMD float32 exp differs from it by a few float32 ulp - the reference's own last bits).
__device__ __forceinline__ float esat_x_f32(float ta, float a3, float a4) {
    return 611.21f * expf(a3 * (ta - 273.16f) / (ta - a4));
}
// the expression as written (:91-105): both phases, IEEE divisions, the library's expf
__device__ __forceinline__ float esat_mixed_f32_literal(float ta) {
    const float T0 = 273.16f, Ti = 250.16f;
    float alpha = __builtin_nanf("");
    if (ta >= T0) alpha = 1.0f;
    if (ta <= Ti) alpha = 0.0f;
    if (ta < T0 && ta > Ti) { const float r = (ta - Ti) / 23.0f; alpha = r * r; }   // (T0 - Ti) = 23.000000000000028 -> 23.0f
    return alpha * esat_x_f32(ta, 17.502f, 32.19f) + (1.0f - alpha) * esat_x_f32(ta, 22.587f, -0.7f);
}
// n / d in float32 by the compiler's own IEEE sequence without v_div_scale (x2) and v_div_fixup: v_rcp_f32, one Newton
// step, q = n r, two residual corrections - 8 instead of 11 instructions and the same bits whenever neither operand
// needs scaling (div_ns above is the float64 form).  Used for a3 (T - T0) / (T - a4) with 60 K < T < 10^4 K.
__device__ __forceinline__ float div_ns_f32(float n, float d) {
    float r = __builtin_amdgcn_rcpf(d);
    r = __builtin_fmaf(__builtin_fmaf(-d, r, 1.0f), r, r);
    float q = n * r;
    q = __builtin_fmaf(__builtin_fmaf(-d, q, n), r, q);
    return __builtin_fmaf(__builtin_fmaf(-d, q, n), r, q);
}
// the device library's expf arithmetic - x log2(e) as a float32 pair, n = rint, v_exp_f32 of the remainder, ldexp -
// without its two range selects (callers keep |x| < 87): the same bits as expf() there
// (tests/...::test_reference_mode_esat_f32_fast_path_is_the_literal_expression)
__device__ __forceinline__ float pgw_expf_core(float x) {
    const float log2e = 0x1.715476p+0f;                        // 0x3fb8aa3b
    const float ph = x * log2e;
    float pl = __builtin_fmaf(x, log2e, -ph);
    pl = __builtin_fmaf(x, __uint_as_float(0x32a5705fu), pl);   // + x * (log2(e) - float(log2(e)))
    const float n = __builtin_rintf(ph);
    const float a = (ph - n) + pl;
    return __builtin_ldexpf(__builtin_amdgcn_exp2f(a), (int)n);
}
__device__ __forceinline__ float no_speculate_f(float x) {
    asm volatile("" : "+v"(x));
    return x;
}
// alpha e_w + (1 - alpha) e_i for alpha in {0, 1} is exactly the phase the temperature needs: the dropped term is
// 0 * finite = +0 and x + 0 = x in float32 as in float64 (esat_mixed above).  One division and one exponential for
// T >= T0 (water) and for 60 K < T <= Ti (ice); mixed phase, colder than 60 K (e_i approaches the float32 denormals,
// e_w overflows below 32.19 K), hotter than 10^4 K and NaN take the literal expression behind ONE divergent region.
__device__ __forceinline__ float esat_mixed_f32(float ta) {
#ifdef PGW_ESAT_F32_LITERAL                                      // A/B knob: round 2's form
    return esat_mixed_f32_literal(ta);
#endif
    const float T0 = 273.16f, Ti = 250.16f;
    const bool warm = (ta >= T0);
    const float a3 = warm ? 17.502f : 22.587f;
    const float a4 = warm ? 32.19f : -0.7f;
    float e1 = 611.21f * pgw_expf_core(div_ns_f32(a3 * (ta - T0), ta - a4));
    if (__builtin_expect(!((warm && ta < 1.0e4f) || (ta <= Ti && ta > 60.0f)), 0)) e1 = esat_mixed_f32_literal(no_speculate_f(ta));
    return e1;
}
// hus float32, pa float64 (ak/bk are float64): hus*pa is float64, the denominator CON_MW_MD + 0.378*hus float32 (:63).
// The two float64 quotients through div_ns (divisors of known range: 0.622 + 0.378 q, e_sat; without the v_div_fixup that
// q_to_e / q_to_rh above add).
__device__ __forceinline__ double q_to_rh_f32_literal(float hus, double pa, float ta);
__device__ __forceinline__ double q_to_rh_f32(float hus, double pa, float ta) {
#ifdef PGW_ESAT_F32_LITERAL
    return q_to_rh_f32_literal(hus, pa, ta);
#endif
    const double vapp = div_ns((double)hus * pa, (double)(0.622f + 0.378f * hus));
    return div_ns(vapp, (double)esat_mixed_f32(ta)) * 100;
}
__device__ __forceinline__ double q_to_rh_f32_literal(float hus, double pa, float ta) {
    const double vapp = (double)hus * pa / (double)(0.622f + 0.378f * hus);
    return (vapp / (double)esat_mixed_f32_literal(ta)) * 100;
}

__device__ __forceinline__ double div_by_100(double x) { return SharedDivisor(100.0, 0.01).divide(x); }
__device__ __forceinline__ double rh_to_e(double hur, double ta) {         // :123
    return div_by_100(hur) * esat_mixed(ta);
}
__device__ __forceinline__ double rh_to_q(double hur, double pa, double ta) {   // :118-125
    return e_to_q(rh_to_e(hur, ta), pa);
}

// ---- settings.function_dtype_flow = 'reference': functions.py:58-125 in numpy's promoted type at every node ----
// float (op) float -> float, float (op) double -> double: C++'s usual arithmetic conversions are numpy's lattice for
// float32 / float64 arrays, and a python-float constant takes the type of the array it meets (written T(c) below).
// Every float32 node is one IEEE operation (-ffp-contract=off, correctly rounded float32 division); e_sat runs wholly in
// the type of `ta` (esat_mixed_f32 / esat_mixed above, which both evaluate :91-105 as written).
template <typename A, typename B> using promo_t = decltype(A() + B());
// result type of humidity_expr<WHICH> below
template <int WHICH, typename TA, typename TB, typename TC>
using humidity_out_t = std::conditional_t<(WHICH >= 2 && WHICH <= 4), TA,
                                          std::conditional_t<(WHICH <= 1), promo_t<TA, TB>, promo_t<promo_t<TA, TB>, TC>>>;
__device__ __forceinline__ float esat_x_t(float ta, bool water) {
    return water ? esat_x_f32(ta, 17.502f, 32.19f) : esat_x_f32(ta, 22.587f, -0.7f);
}
__device__ __forceinline__ double esat_x_t(double ta, bool water) {               // the literal form of k_humidity_leaf
    return water ? 611.21 * pgw_exp(17.502 * (ta - 273.16) / (ta - 32.19)) : 611.21 * pgw_exp(22.587 * (ta - 273.16) / (ta - (-0.7)));
}
__device__ __forceinline__ float esat_mixed_t(float ta) { return esat_mixed_f32(ta); }
__device__ __forceinline__ double esat_mixed_t(double ta) { return esat_mixed(ta); }
// WHICH 0: q -> e (:58-64; a = hus, b = pa)   1: e -> q (:66-72; a = vapp, b = pa)   2 / 3: e_sat over water / ice (:74-89; a = ta)
// 4: mixed-phase e_sat (:91-105; a = ta)      5: q -> RH (:107-116; hus, pa, ta)    6: RH -> q (:118-125; hur, pa, ta)
template <int WHICH, typename TA, typename TB, typename TC>
__device__ __forceinline__ auto humidity_expr(TA a, TB b, TC c) {
    if constexpr (WHICH == 0) return a * b / (TA(CON_MW_MD) + TA(0.378) * a);
    else if constexpr (WHICH == 1) return TA(CON_MW_MD) * a / (b - TA(1 - CON_MW_MD) * a);
    else if constexpr (WHICH == 2) return esat_x_t(a, true);
    else if constexpr (WHICH == 3) return esat_x_t(a, false);
    else if constexpr (WHICH == 4) return esat_mixed_t(a);
    else if constexpr (WHICH == 5) {
        // the mix a float32 file produces (float32 QV and T, float64 pressure) and the uniform float64 one through the
        // helpers the file kernels use: the same expression with the scale-free quotients (div_ns: same bits)
        if constexpr (sizeof(TA) == 4 && sizeof(TB) == 8 && sizeof(TC) == 4) return q_to_rh_f32(a, b, c);
        else if constexpr (sizeof(TA) == 8 && sizeof(TB) == 8 && sizeof(TC) == 8) return q_to_rh(a, b, c);
        else {
            const auto r = humidity_expr<0>(a, b, c) / esat_mixed_t(c);
            return r * decltype(r)(100);
        }
    } else {
        if constexpr (sizeof(TA) == 8 && sizeof(TB) == 8 && sizeof(TC) == 8) return rh_to_q(a, b, c);
        else {
            const auto vapp = a / TA(100) * esat_mixed_t(c);
            return humidity_expr<1>(vapp, b, c);
        }
    }
}

// V elements of T as themselves (no widening), at most 16 bytes per access
template <typename T, int V>
__device__ __forceinline__ void loadv_typed(const T *__restrict__ p, T (&out)[V]) {
    constexpr int H = (sizeof(T) * V <= 16) ? V : (int)(16 / sizeof(T));
#pragma unroll
    for (int h = 0; h < V; h += H) {
        Pack<T, H> t = *reinterpret_cast<const Pack<T, H> *>(p + h);
#pragma unroll
        for (int i = 0; i < H; ++i) out[h + i] = t.v[i];
    }
}
template <typename T, int V>
__device__ __forceinline__ void storev_typed(T *__restrict__ p, const T (&in)[V]) {
    constexpr int H = (sizeof(T) * V <= 16) ? V : (int)(16 / sizeof(T));
#pragma unroll
    for (int h = 0; h < V; h += H) {
        Pack<T, H> t;
#pragma unroll
        for (int i = 0; i < H; ++i) t.v[i] = in[h + i];
        *reinterpret_cast<Pack<T, H> *>(p + h) = t;
    }
}

// functions.py:135  pa_hl.where(pa_hl > 0, 0.0001): NaN > 0 is False -> 1e-4
__device__ __forceinline__ double fix_p(double p) { return (p > 0) ? p : 0.0001; }

// ordered-bits view of a non-negative (or any positive) double for atomicMax/atomicMin
__device__ __forceinline__ unsigned long long dbits(double x) { return (unsigned long long)__double_as_longlong(x); }

__device__ __forceinline__ double wave_max(double x) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) x = fmax(x, __shfl_xor(x, off, 64));
    return x;
}
__device__ __forceinline__ double wave_min(double x) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) x = fmin(x, __shfl_xor(x, off, 64));
    return x;
}

}  // namespace pgw
