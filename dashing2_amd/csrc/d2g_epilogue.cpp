// d2g_epilogue.cpp -- everything of the host half that turns the device's integer counts into values: the (gt, lt), neq and lut
// epilogues of compare() with their upper-triangle form, register truncation (d2g_regs_truncate) and the truncated epilogues, the
// exact-set epilogues and `contain`'s table.  Compiled with g++ (not hipcc) so that `long double` is the 80-bit x87 type the
// reference's gcc build uses; the goldens compare bit for bit.
//
// Reference lines restated here are cited per function.
#include "../../include/d2g.h"
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

// cmp_core.cpp:361, the generic lambda `(auto x) -> double`.  T matters: 2. * x / (1. + x), the logarithm and the product are
// evaluated in T (float widens to double, long double stays x87), with one rounding to double on return.
template <class T> static inline double sim2dist(T x, int k) {
    return x ? std::log(2. * x / (1. + x)) * (-1. / std::max(1, k)) : std::numeric_limits<double>::infinity();
}
// cmp_core.cpp:573-575
static inline float finish(long double ret) {
    if (std::isnan(ret) || std::isinf(ret)) ret = std::numeric_limits<long double>::max();
    return float(ret);
}

// The pair walks behind every matrix epilogue: f(p, i, j) for pair (i, j) at position p of the output.
// Rows [r0, r1) of the condensed upper triangle of an N x N matrix, j > i:
template <class F> static inline void walk_ut(size_t N, size_t r0, size_t r1, int nthreads, F f) {
    std::vector<size_t> off(r1 - r0 + 1, 0);
    for (size_t i = r0; i < r1; ++i) off[i - r0 + 1] = off[i - r0] + (N - 1 - i);
    if (nthreads < 1) nthreads = 1;
#ifdef _OPENMP
    #pragma omp parallel for schedule(dynamic, 4) num_threads(nthreads)
#endif
    for (size_t i = r0; i < r1; ++i) {
        const size_t base = off[i - r0];
        for (size_t j = i + 1; j < N; ++j) f(base + (j - i - 1), i, j);
    }
}
// ... and a row-major block, rows [a0, a1) x columns [b0, b1):
template <class F> static inline void walk_rect(size_t a0, size_t a1, size_t b0, size_t b1, int nthreads, F f) {
    if (nthreads < 1) nthreads = 1;
    const size_t w = b1 - b0;
#ifdef _OPENMP
    #pragma omp parallel for schedule(dynamic, 4) num_threads(nthreads)
#endif
    for (size_t i = a0; i < a1; ++i)
        for (size_t j = b0; j < b1; ++j) f((i - a0) * w + (j - b0), i, j);
}

// cmp_core.cpp:323-325
static inline long double g_b(long double b, long double arg) { return (1.L - std::pow(b, -arg)) / (1.L - 1.L / b); }

// compressed branch of compare(), setsketch: cmp_core.cpp:425-448, from alpha = g_b(b, gt/S) and beta = g_b(b, lt/S)
static inline float trunc_gtlt_from(long double alpha, long double beta, long double lhcard, long double rhcard, int measure, int k) {
    long double mu;
    if (alpha + beta >= 1.) mu = lhcard + rhcard;
    else mu = std::max((lhcard + rhcard) / (2.L - alpha - beta), 0.L);
    long double ret = std::max(1.L - (alpha + beta), 0.L);
    switch (measure) {
        case D2G_INTERSECTION: ret *= mu; break;
        case D2G_UNION_SIZE: ret = lhcard + rhcard - (ret * mu); break;
        case D2G_CONTAINMENT: ret = ret * mu / lhcard; break;
        case D2G_SYMMETRIC_CONTAINMENT: ret = (ret * mu) / std::min(lhcard, rhcard); break;
        case D2G_POISSON_LLR: ret = sim2dist(ret, k); break;
        default: ;
    }
    return finish(ret);
}

// g_b(b, c/S) takes S+1 values: one table per run, no powl per pair
static std::vector<long double> g_b_table(size_t S, long double b) {
    std::vector<long double> t(S + 1);
    const long double invdenom = 1.L / S;
    for (size_t c = 0; c <= S; ++c) t[c] = g_b(b, c * invdenom);
    return t;
}

static void trunc_fail(char *err, size_t cap, const char *msg) { if (err && cap) std::snprintf(err, cap, "%s", msg); }

extern "C" {

// cmp_core.cpp:458-494
float d2g_epilogue_gtlt(uint64_t gt, uint64_t lt, size_t S, double lhc, double rhc, int measure, int k) {
    long double ret = std::numeric_limits<float>::max();
    const long double invdenom = 1.L / S;
    const long double alpha = gt * invdenom, beta = lt * invdenom;
    const long double lhcard = lhc, rhcard = rhc;
    long double eq = (1. - alpha - beta);
    const long double ucard = std::max((lhcard + rhcard) / (2.L - alpha - beta), 0.L);
    if (eq <= 0.)
        return measure != D2G_POISSON_LLR ? 0.f : std::numeric_limits<float>::infinity();
    static constexpr long double EPS = 1e-15;
    if (eq <= EPS) eq = 0;
    const float isz = ucard * eq, sim = eq;
    switch (measure) {
        case D2G_SIMILARITY: ret = sim; break;
        case D2G_INTERSECTION: ret = isz; break;
        case D2G_CONTAINMENT: ret = isz / rhcard; break;
        case D2G_SYMMETRIC_CONTAINMENT: ret = isz / std::min(lhcard, rhcard); break;
        case D2G_POISSON_LLR: ret = sim2dist(sim, k); break;
        case D2G_UNION_SIZE: ret = lhcard + rhcard - isz; break;
        default: ret = -1.f; break;
    }
    return finish(ret);
}

// cmp_core.cpp:495-517
float d2g_epilogue_neq(uint64_t neq, size_t S, double lhc, double rhc, int measure, int k) {
    const long double lhcard = lhc, rhcard = rhc, invdenom = 1.L / S;
    long double ret = invdenom * neq;
    auto ucard = [&]() { return std::max((lhcard + rhcard) / (1.L + ret), 0.L); };
    if (measure == D2G_INTERSECTION) ret *= ucard();
    else if (measure == D2G_SYMMETRIC_CONTAINMENT) ret *= ucard() / std::min(lhcard, rhcard);
    else if (measure == D2G_CONTAINMENT) ret *= ucard() / lhcard;
    else if (measure == D2G_POISSON_LLR) ret = sim2dist(ret, k);
    else if (measure == D2G_UNION_SIZE) {
        const long double isz = ret * ucard();
        ret = lhcard + rhcard - isz;
    }
    return finish(ret);
}

int d2g_epilogue_lut(size_t S, int measure, int k, int multiset_space, float *lut) {
    if (!lut || !S) return D2G_ERR_INVALID;
    if (measure != D2G_SIMILARITY && measure != D2G_POISSON_LLR) return D2G_ERR_UNSUPPORTED;
    if (multiset_space) {
        for (size_t e = 0; e <= S; ++e) lut[e] = d2g_epilogue_neq(e, S, 1., 1., measure, k);
        return D2G_OK;
    }
    // set space: the value is a function of gt and lt; it depends on gt+lt only when every
    // product gt * (1.L/S) is exact, i.e. S is a power of two.
    if (S & (S - 1)) return D2G_ERR_UNSUPPORTED;
    for (size_t e = 0; e <= S; ++e) lut[e] = d2g_epilogue_gtlt(S - e, 0, S, 1., 1., measure, k);
    return D2G_OK;
}

// epilogue over rows [r0,r1) of the condensed upper triangle from the device's integer counts.
// ca = neq (or gt when cb != null), cb = lt.  Same arithmetic as compare(): cmp_core.cpp:458-517.
int d2g_epilogue_ut(const uint32_t *ca, const uint32_t *cb, const double *cards, size_t N, size_t S,
                    size_t r0, size_t r1, int measure, int k, int multiset_space, int nthreads, float *out) {
    if (r0 > r1 || r1 > N || !S) return D2G_ERR_INVALID;
    if (d2g_ut_count(N, r0, r1) == 0) return D2G_OK;
    if (!ca || !cards || !out) return D2G_ERR_INVALID;
    walk_ut(N, r0, r1, nthreads, [=](size_t p, size_t i, size_t j) {
        if (multiset_space) out[p] = d2g_epilogue_neq(ca[p], S, cards[i], cards[j], measure, k);
        else if (cb) out[p] = d2g_epilogue_gtlt(ca[p], cb[p], S, cards[i], cards[j], measure, k);
        // power-of-two S: every multiple of 1/S is exact, so only gt+lt = S-neq matters
        else out[p] = d2g_epilogue_gtlt(S - ca[p], 0, S, cards[i], cards[j], measure, k);
    });
    return D2G_OK;
}

// ---- truncated registers (--fastcmp <4|2|1>, --bbit-sigs): make_compressed, cmp_core.cpp:209-322
int d2g_regs_truncate(const double *sigs, size_t n, size_t S, int regbytes, int bbit, void *codes_out, long double *ab_out,
                      double *minmax_out, int nthreads, char *err, size_t errcap) {
    if (err && errcap) err[0] = 0;
    if (regbytes != 1 && regbytes != 2 && regbytes != 4) { trunc_fail(err, errcap, "regs_truncate: register size must be 1, 2 or 4 bytes"); return D2G_ERR_INVALID; }
    if (!sigs || !codes_out || !n || !S) { trunc_fail(err, errcap, "regs_truncate: null or empty matrix"); return D2G_ERR_INVALID; }
    if (nthreads < 1) nthreads = 1;
    const size_t nsigs = n * S;
    uint8_t *c8 = static_cast<uint8_t *>(codes_out);
    uint16_t *c16 = static_cast<uint16_t *>(codes_out);
    uint32_t *c32 = static_cast<uint32_t *>(codes_out);
    auto put = [&](size_t i, uint64_t v) {
        if (regbytes == 4) c32[i] = (uint32_t)v; else if (regbytes == 2) c16[i] = (uint16_t)v; else c8[i] = (uint8_t)v;
    };
    if (bbit) {                                                   // :294-320, reg2sig :19-30
        const int shift = regbytes == 1 ? 58 : regbytes == 2 ? 48 : 32;
        if (ab_out) ab_out[0] = ab_out[1] = 0.L;
#ifdef _OPENMP
        #pragma omp parallel for schedule(static) num_threads(nthreads)
#endif
        for (size_t i = 0; i < nsigs; ++i) {
            uint64_t v;
            std::memcpy(&v, &sigs[i], sizeof(v));
            put(i, d2g_wang_hash(v ^ 0xa3407fb23cd20efull) >> shift);
        }
        return D2G_OK;
    }
    // :246-292
    const long double q = regbytes == 1 ? 254.3 : regbytes == 2 ? 65534 : 4294967294;     // 254.3 is a double constant there, too
    double minreg = std::numeric_limits<double>::max(), maxreg = -std::numeric_limits<double>::max();
    bool has_inf = false;
    for (size_t i = 0; i < nsigs; ++i) {
        const double v = sigs[i];
        if (v <= 0 || v == std::numeric_limits<double>::max()) continue;
        if (std::isinf(v)) has_inf = true;
        minreg = std::min(minreg, v);
        maxreg = std::max(maxreg, v);
    }
    if (has_inf) { trunc_fail(err, errcap, "regs_truncate: a register is +inf"); return D2G_ERR_INVALID; }
    if (maxreg < minreg) { trunc_fail(err, errcap, "regs_truncate: the matrix holds no finite positive register"); return D2G_ERR_INVALID; }
    // CSetSketch::optimal_parameters (setsketch.h:563-566, called with (min, max): swapped) -> setsketch.cpp:7-10
    const long double hi = maxreg, lo = minreg;
    const long double b = std::exp(std::log(hi / lo) / q);
    const long double a = hi / b;
    if (minmax_out) { minmax_out[0] = minreg; minmax_out[1] = maxreg; }
    if (!(a > 0.L) || !(b > 0.L) || std::isinf(a) || std::isinf(b)) {
        trunc_fail(err, errcap, "regs_truncate: setsketch parameters a, b are not finite and positive");
        return D2G_ERR_INVALID;
    }
    if (ab_out) { ab_out[0] = a; ab_out[1] = b; }
    const long double logbinv = 1.L / std::log1p(b - 1.L);
    const int64_t top = int64_t(q + 1);
#ifdef _OPENMP
    #pragma omp parallel for schedule(static) num_threads(nthreads)
#endif
    for (size_t i = 0; i < nsigs; ++i) {
        const long double sub = 1.L - std::log(static_cast<long double>(sigs[i]) / a) * logbinv;
        // a value outside int64 (log(0) = -inf -> sub = +inf) converts to the x86 "integer indefinite", INT64_MIN, which clamps to 0
        const int64_t cast = (sub >= -0x1p63L && sub < 0x1p63L) ? static_cast<int64_t>(sub) : std::numeric_limits<int64_t>::min();
        put(i, (uint64_t)std::max(int64_t(0), std::min(top, cast)));
    }
    return D2G_OK;
}

// compressed branch of compare(), b-bit: cmp_core.cpp:406-423
float d2g_epilogue_trunc_neq(uint64_t neq, size_t S, int regbytes, double lhc, double rhc, int measure, int k) {
    const long double lhcard = lhc, rhcard = rhc, invdenom = 1.L / S;
    const long double b2pow = -std::ldexp(1.L, -(regbytes * 8));
    long double ret = std::max(0.L, std::fma((long double)neq, invdenom, b2pow) / (1.L + b2pow));
    auto ucard = [&]() { return std::max((lhcard + rhcard) / (2.L - (1.L - ret)), 0.L); };
    if (measure == D2G_INTERSECTION || measure == D2G_UNION_SIZE) {
        const long double isz = ucard();
        ret = measure == D2G_INTERSECTION ? isz : lhcard + rhcard - isz;
    } else if (measure == D2G_CONTAINMENT) ret = ucard() * ret / lhcard;
    else if (measure == D2G_POISSON_LLR) ret = sim2dist(ret, k);
    else if (measure == D2G_SYMMETRIC_CONTAINMENT) ret = ucard() * ret / std::min(lhcard, rhcard);
    return finish(ret);
}

float d2g_epilogue_trunc_gtlt(uint64_t gt, uint64_t lt, size_t S, const long double *b, double lhc, double rhc, int measure, int k) {
    const long double invdenom = 1.L / S;
    return trunc_gtlt_from(g_b(*b, gt * invdenom), g_b(*b, lt * invdenom), lhc, rhc, measure, k);
}

// ca = neq (b == NULL: b-bit codes) or gt with cb = lt (setsketch codes with base *b)
int d2g_epilogue_trunc_ut(const uint32_t *ca, const uint32_t *cb, const double *cards, size_t N, size_t S, size_t r0, size_t r1,
                          int measure, int k, int regbytes, const long double *b, int nthreads, float *out) {
    if (r0 > r1 || r1 > N || !S) return D2G_ERR_INVALID;
    if (d2g_ut_count(N, r0, r1) == 0) return D2G_OK;
    if (!ca || !cards || !out || (b && !cb)) return D2G_ERR_INVALID;
    std::vector<long double> gbv;
    if (b) gbv = g_b_table(S, *b);
    const long double *gb = gbv.data();
    walk_ut(N, r0, r1, nthreads, [=](size_t p, size_t i, size_t j) {
        if (!b) out[p] = d2g_epilogue_trunc_neq(ca[p], S, regbytes, cards[i], cards[j], measure, k);
        else if (ca[p] > S || cb[p] > S) out[p] = std::numeric_limits<float>::quiet_NaN();     // not counts of S registers
        else out[p] = trunc_gtlt_from(gb[ca[p]], gb[cb[p]], cards[i], cards[j], measure, k);
    });
    return D2G_OK;
}

// the same over a row-major block: rows [a0,a1) x columns [b0,b1) of the N x N matrix, compare(row, column)
int d2g_epilogue_trunc_rect(const uint32_t *ca, const uint32_t *cb, const double *cards, size_t N, size_t S, size_t a0, size_t a1,
                            size_t b0, size_t b1, int measure, int k, int regbytes, const long double *b, int nthreads, float *out) {
    if (a0 > a1 || a1 > N || b0 > b1 || b1 > N || !S) return D2G_ERR_INVALID;
    if (a0 == a1 || b0 == b1) return D2G_OK;
    if (!ca || !cards || !out || (b && !cb)) return D2G_ERR_INVALID;
    std::vector<long double> gbv;
    if (b) gbv = g_b_table(S, *b);
    const long double *gb = gbv.data();
    walk_rect(a0, a1, b0, b1, nthreads, [=](size_t p, size_t i, size_t j) {
        if (!b) out[p] = d2g_epilogue_trunc_neq(ca[p], S, regbytes, cards[i], cards[j], measure, k);
        else if (ca[p] > S || cb[p] > S) out[p] = std::numeric_limits<float>::quiet_NaN();
        else out[p] = trunc_gtlt_from(gb[ca[p]], gb[cb[p]], cards[i], cards[j], measure, k);
    });
    return D2G_OK;
}

// ---- exact k-mer sets (--set, --countdict): the exact branch of compare(), cmp_core.cpp:518-575
// CORRECT_RES (:519-526) on `double res = isz_size` (:559), assigned to the long double ret, then :573-575.  UNION_SIZE has no arm
// there and falls through to the intersection; here it is the union weighted_compare computed and compare() dropped.
float d2g_epilogue_exact(uint64_t isz, double lhc, double rhc, int measure, int k) {
    double res = (double)isz;
    if (measure == D2G_SYMMETRIC_CONTAINMENT) res = res / std::min(lhc, rhc);
    else if (measure == D2G_POISSON_LLR || measure == D2G_SIMILARITY) {
        res = res / (lhc + rhc - res);
        if (measure == D2G_POISSON_LLR) res = sim2dist(res, k);
    } else if (measure == D2G_CONTAINMENT) res /= lhc;
    else if (measure == D2G_UNION_SIZE) res = lhc + rhc - res;
    return finish(res);
}

int d2g_epilogue_exact_ut(const uint64_t *isz, const double *cards, size_t N, size_t r0, size_t r1, int measure, int k, int nthreads,
                          float *out) {
    if (r0 > r1 || r1 > N) return D2G_ERR_INVALID;
    if (d2g_ut_count(N, r0, r1) == 0) return D2G_OK;
    if (!isz || !cards || !out) return D2G_ERR_INVALID;
    walk_ut(N, r0, r1, nthreads, [=](size_t p, size_t i, size_t j) { out[p] = d2g_epilogue_exact(isz[p], cards[i], cards[j], measure, k); });
    return D2G_OK;
}

int d2g_epilogue_exact_rect(const uint64_t *isz, const double *cards, size_t N, size_t a0, size_t a1, size_t b0, size_t b1, int measure,
                            int k, int nthreads, float *out) {
    if (a0 > a1 || a1 > N || b0 > b1 || b1 > N) return D2G_ERR_INVALID;
    if (a0 == a1 || b0 == b1) return D2G_OK;
    if (!isz || !cards || !out) return D2G_ERR_INVALID;
    walk_rect(a0, a1, b0, b1, nthreads, [=](size_t p, size_t i, size_t j) { out[p] = d2g_epilogue_exact(isz[p], cards[i], cards[j], measure, k); });
    return D2G_OK;
}

// contain's table (src/contain_main.cpp:221,237-241): `cmatptr[j] = ssiv * matches[j]` is a double product narrowed to float,
// `cstatsptr[j] = matchsums[j] / matches[j]` the quotient of two uint32 -- the floor of the mean depth -- converted to float
int d2g_epilogue_contain(const uint32_t *matches, const uint32_t *matchsums, size_t n, size_t S, float *coverage, float *depth) {
    if (S == 0 || (n && (!matches || !matchsums || !coverage || !depth))) return D2G_ERR_INVALID;
    const double ssiv = 1. / double(S);
    for (size_t i = 0; i < n; ++i) {
        coverage[i] = matches[i] ? float(ssiv * matches[i]) : 0.f;
        depth[i] = matches[i] ? float(matchsums[i] / matches[i]) : 0.f;
    }
    return D2G_OK;
}

}  // extern "C"
