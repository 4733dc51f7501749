// d2g_k3_device.h -- the device code that kernels of more than one unit of K3 share: the compact key maps (bucketing stores by them,
// counting reads by them), the BMH-D2G process machinery (the main pass walks count tables with it, the list kernels explicit sets),
// block_hmax, genome_of_bucket and bmh_guess, which host and device must compute alike.  Everything stays internal to the unit that
// includes it.
#pragma once
#include "d2g_k3.h"

namespace {

constexpr int K3_MAXB = 1 << K3_MAXBBITS;   // buckets per genome (LDS histogram)
constexpr int BMH_STACK = 72;

// ---------------------------------------------------------------------------------------------
// COMPACT path (DNA k <= 21 -- key bits d2g_key_bits(k, alphabet) <= 42 --, D2G_K3_COMPACT=1): the multi-split stores 4 bytes per k-mer and writes them coalesced.
//
// Counting only needs a key that identifies the k-mer, so the split works on the 2k-bit k-mer x itself (the
// masked key Wang(x ^ XORMASK) is a bijection of it and is computed once per DISTINCT k-mer in the main pass).
// x = hi:lo with lo = 32 bits, hi = key bits - 32 <= 10 bits (DNA: 2k - 32).  With m = lo * 0x9E3779B1 and t = the top bb bits of m,
//     bucket = t ^ (hi << (bb - hb))                           (bb >= hb bucket bits per genome)
// hi is recovered from (bucket, lo), so a bucket stores lo only; and within a bucket lo identifies the k-mer.
// Lower bits of m select sub-ranges and table rounds.
//
// The generic scatter issues one 8-byte store per k-mer to 4096 write fronts: 1.25e9 scattered stores take 11.5 ms
// whatever their width (measured: 13.6 ms with 4-byte stores, 2.9 ms with none) and reach HBM as 38 GB for 10 GB
// of keys.  Here a workgroup sorts each tile of 16 384 k-mers by bucket in LDS first (<= 1024 buckets: runs of
// ~16 keys = 64 B) and then flushes the tile with consecutive lanes writing consecutive words.  The per-tile
// bucket counts come from the histogram pass (u16 per tile and bucket), the scan turns them into per-tile write
// offsets: no atomics on global memory, two enumerations of the k-mers in total.
// ---------------------------------------------------------------------------------------------
constexpr int K3C_MAXBBITS = 10;
constexpr int K3C_MAXB = 1 << K3C_MAXBBITS;
constexpr int K3C_TILE = K1_THREADS * K1_CHUNK;       // k-mers of one pass of a workgroup
constexpr int K3C_TARGET = 4096;                      // mean k-mers per bucket aimed for (3-4 table rounds)
constexpr uint32_t K3C_MUL = 0x9E3779B1u;
static_assert(K3C_TILE <= 65535 + 1, "per-tile bucket counts are stored as u16 (a count of 65536 cannot occur: see k3c_hist)");

__device__ __forceinline__ uint32_t k3c_mix(uint32_t lo) { return lo * K3C_MUL; }
__device__ __forceinline__ uint32_t k3c_bucket(uint64_t x, uint32_t bb, uint32_t hb) {
    const uint32_t lo = (uint32_t)x, hi = (uint32_t)(x >> 32);
    const uint32_t t = bb ? k3c_mix(lo) >> (32 - bb) : 0u;
    return t ^ (hi << (bb - hb));
}
// the k-mer of stored word lo in bucket b (local index) of a genome with bb bucket bits
__device__ __forceinline__ uint64_t k3c_kmer(uint32_t lo, uint32_t b, uint32_t bb, uint32_t hb) {
    const uint32_t t = bb ? k3c_mix(lo) >> (32 - bb) : 0u;
    const uint32_t hi = hb ? (b ^ t) >> (bb - hb) : 0u;
    return ((uint64_t)hi << 32) | lo;
}

// ---------------------------------------------------------------------------------------------
// BMH-D2G process machinery (spec: DESIGN.md; sequential twin: oracle/d2_bmh_oracle.c)
// ---------------------------------------------------------------------------------------------
struct Proc {
    uint64_t p, q;       // weight-level range [V(p), V(q)), double bit patterns
    double x;            // time of the current point
    uint64_t rng;        // wyhash64_stateless state (in-tree twin: reference src/ssi.h:26-36)
    uint32_t i;          // register of the current point
    uint32_t pad;
};

__device__ __forceinline__ double V(uint64_t l) { return __longlong_as_double((long long)l); }
__device__ __forceinline__ uint64_t dbits(double d) { return (uint64_t)__double_as_longlong(d); }

__device__ __forceinline__ uint64_t wy_next(uint64_t &s) {
    s += 0x60bee2bee120fc15ull;
    const uint64_t a = s ^ 0xe7037ed1a0b428dbull;
    return (a * s) ^ __umul64hi(a, s);
}

// natural log on [2^-53, 1] in plain IEEE double ops (no FMA contraction: -ffp-contract=off), the
// same operation sequence as d2o_dlog
__device__ __forceinline__ double dlog(double u) {
    const double ln2_hi = 6.93147180369123816490e-01, ln2_lo = 1.90821492927058770002e-10,
                 Lg1 = 6.666666666666735130e-01, Lg2 = 3.999999999940941908e-01, Lg3 = 2.857142874366239149e-01,
                 Lg4 = 2.222219843214978396e-01, Lg5 = 1.818357216161805012e-01, Lg6 = 1.531383769920937332e-01,
                 Lg7 = 1.479819860511658591e-01;
    const uint64_t b = dbits(u);
    int e = (int)(b >> 52) - 1023;
    double m = V((b & 0x000FFFFFFFFFFFFFull) | 0x3FF0000000000000ull);
    if (m > 1.4142135623730951) { m = m * 0.5; e += 1; }
    const double f = m - 1.0;
    const double s = f / (2.0 + f);
    const double z = s * s;
    const double R = z * (Lg1 + z * (Lg2 + z * (Lg3 + z * (Lg4 + z * (Lg5 + z * (Lg6 + z * Lg7))))));
    const double hfsq = 0.5 * f * f;
    const double dk = (double)e;
    return dk * ln2_hi - ((hfsq - (s * (hfsq + R) + dk * ln2_lo)) - f);
}

// advance to the process's next point; false = certainly later than `bound` (drop the process).
// Early-out: -log(u) >= 1 - u, so (1-u)/width > bound already proves x > bound without the log
// and the division (the 1e-9 margin dwarfs every rounding involved).
__device__ __forceinline__ bool proc_next(Proc &P, uint32_t m, double bound) {
    const double width = V(P.q) - V(P.p);
    const uint64_t r1 = wy_next(P.rng);
    const double uu = (double)((r1 >> 11) + 1) * 0x1p-53;            // (0, 1]
    if ((1.0 - uu) > bound * width * 1.000000001) { return false; }
        const double E = -dlog(uu);
    P.x = P.x + E / width;
    const uint64_t r2 = wy_next(P.rng);
    P.i = (uint32_t)__umul64hi(r2, (uint64_t)m);
    return P.x <= bound;
}

__device__ __forceinline__ void reg_min(uint64_t *h, uint32_t i, double x) {
    const uint64_t xb = dbits(x);
    if (xb < h[i]) atomicMin((unsigned long long *)&h[i], (unsigned long long)xb);
}
// second pass over FINAL registers: which element set each register (BagMinHash2::ids(), reference
// src/wsketch.cpp:66-67).  Ties (two elements with the same point) go to the smaller position.
struct ArgSink {
    const uint64_t *h;   // final registers of the set
    uint64_t *arg;       // [m] position of the element that owns the register, pre-set to ~0
    uint64_t pos;        // position of the element being walked
};
__device__ __forceinline__ void reg_min(const ArgSink &s, uint32_t i, double x) {
    if (dbits(x) == s.h[i]) atomicMin((unsigned long long *)&s.arg[i], (unsigned long long)s.pos);
}

// locate P's current point: narrow P to the half that holds it, level by level; the other half
// becomes a fresh process starting at P.x.  Pushes what may still matter.
// The expensive half of proc_next (log + division) is NOT done inside the level loop: a sibling
// that survives the cheap early-out is parked on the stack with its uniform in .x, and all parked
// processes are finished after the loop, where the lanes of a wave are converged again (inside
// the loop each lane would hit the expensive branch at a different level and the wave would pay
// for it once per level).  Same arithmetic in a different order: identical results.
template <class H>
__device__ void bmh_locate(Proc P, uint64_t d, double w, uint32_t m, double bound, H h, Proc *stk, int &sp, int *status) {
    const int sp0 = sp;
    bool counted = false, relevant = true;
    auto park = [&](Proc &S) {
        const double width = V(S.q) - V(S.p);
        const uint64_t r1 = wy_next(S.rng);
        const double uu = (double)((r1 >> 11) + 1) * 0x1p-53;        // (0, 1]
        if ((1.0 - uu) > bound * width * 1.000000001) return;   // see proc_next
        S.x = uu;
        if (sp >= BMH_STACK) { atomicExch(status, K3_STACK_OVERFLOW); return; }        // cannot happen (<= one sibling per tree level); never silent
        stk[sp++] = S;
    };
    for (;;) {
        if (!counted && V(P.q) <= w) { reg_min(h, P.i, P.x); counted = true; }
        if (P.q - P.p <= 1) break;
                const uint64_t r = P.p + ((P.q - P.p) >> 1);
        const uint64_t rb = wy_next(P.rng);
        const double ub = (double)(rb >> 11) * 0x1p-53;              // [0, 1)
        const double vp = V(P.p), vq = V(P.q), vr = V(r);
        const bool left = ub * (vq - vp) < (vr - vp);
        Proc S;
        S.x = 0.; S.i = 0; S.pad = 0;
        S.rng = d ^ (r * 0x9E3779B97F4A7C15ull) ^ 0xD6E8FEB86659FD93ull;
        if (left) { S.p = r; S.q = P.q; P.q = r; }
        else      { S.p = P.p; S.q = r; P.p = r; }
        if (V(S.p) < w) park(S);
        if (!(V(P.p) < w)) { relevant = false; break; }
    }
    if (relevant) park(P);                                           // single-level strip: its next point
    int out = sp0;
    for (int j = sp0; j < sp; ++j) {
        Proc S = stk[j];
                const double E = -dlog(S.x);
        S.x = P.x + E / (V(S.q) - V(S.p));
        const uint64_t r2 = wy_next(S.rng);
        S.i = (uint32_t)__umul64hi(r2, (uint64_t)m);
        if (S.x <= bound) { stk[out++] = S; }
    }
    sp = out;
}

// BMH-D2G top level: 65 fixed strips of [0, 2^53) -- 16 unit strips, then octaves -- each an
// independent Poisson process from time 0 (see oracle/d2_bmh_oracle.c).  A k-mer seen once costs
// one seed, one generator step and one compare.
constexpr int BMH_NTOP = 65;
__device__ __forceinline__ double top_edge(int t) {
    return t <= 16 ? (double)t : V((uint64_t)(1023 + t - 12) << 52);           // 2^(t-12)
}
// number of strips whose lower edge is below w (0 < w <= 2^53): strips 0..top_count(w)-1 are the relevant ones
__device__ __forceinline__ int top_count(double w) {
    if (w <= 16.0) { const int c = (int)w; return c + ((double)c < w); }              // ceil(w)
    const uint64_t b = dbits(w);
    const int e = (int)(b >> 52) - 1023;                                                // floor(log2 w) >= 4
    const int c = 12 + e + ((b & 0x000FFFFFFFFFFFFFull) != 0);                          // edges 2^(t-12) < w  <=>  t < 12 + log2 w
    return c < BMH_NTOP ? c : BMH_NTOP;
}
__device__ __forceinline__ Proc top_proc(uint64_t d, int t) {
    Proc P;
    P.p = dbits(top_edge(t)); P.q = dbits(top_edge(t + 1)); P.x = 0.; P.i = 0; P.pad = 0;
    P.rng = d ^ ((uint64_t)(t + 1) * 0xA0761D6478BD642Full) ^ 0x8EBC6AF09C88C6E3ull;
    return P;
}

// everything below a process whose current point is at or before `bound`
template <class H>
__device__ __forceinline__ void walk_process(const Proc &P0, uint64_t d, double w, uint32_t m, double bound, H h, Proc *stk,
                                             int *status) {
    int sp = 0;
    bmh_locate(P0, d, w, m, bound, h, stk, sp, status);
    while (sp) {
        const Proc Q = stk[--sp];
        if (Q.x <= bound) bmh_locate(Q, d, w, m, bound, h, stk, sp, status);
    }
}

// walk every process of element (d, w) that can still matter under `bound`
template <class H>
__device__ __forceinline__ void walk_element(uint64_t d, double w, uint32_t m, double bound, H h, Proc *stk, int *status) {
    const int nt = top_count(w);
    for (int t = 0; t < nt; ++t) {
        Proc P = top_proc(d, t);
        if (proc_next(P, m, bound)) walk_process(P, d, w, m, bound, h, stk, status);
    }
}

__device__ uint64_t block_hmax(const uint64_t *h, uint32_t m, uint64_t *red) {
    const int tid = threadIdx.x;
    uint64_t v = 0;
    for (uint32_t i = tid; i < m; i += K3_THREADS) { const uint64_t x = h[i]; v = x > v ? x : v; }
    for (int o = 32; o; o >>= 1) { const uint64_t x = __shfl_xor(v, o); v = x > v ? x : v; }
    __syncthreads();
    if ((tid & 63) == 0) red[tid >> 6] = v;
    __syncthreads();
    v = red[0];
    for (int k = 1; k < K3_THREADS / 64; ++k) v = red[k] > v ? red[k] : v;
    return v;
}

__device__ __forceinline__ uint32_t genome_of_bucket(const uint32_t *g_boff, uint32_t n, uint32_t tb) {
    uint32_t lo = 0, hi = n;
    while (hi - lo > 1) { const uint32_t mid = (lo + hi) >> 1; if (g_boff[mid] <= tb) lo = mid; else hi = mid; }
    return lo;
}

// the pruning bound for total weight W: the final maximum register is the max of m exponentials of
// rate W/m -- mean (m/W)(ln m + 0.58), sd 1.28 m/W; 1.25 x (mean + 6 sd) fails about once in 4000 genomes
__host__ __device__ inline double bmh_guess(double W, double m, double lnm) { return 1.25 * (m / W) * (lnm + 0.58 + 8.0); }

}  // namespace
