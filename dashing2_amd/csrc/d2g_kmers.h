// d2g_kmers.h -- device-side k-mer enumeration shared by K1 (OPH) and K3 (k-mer counting):
// the reference's bns::Encoder::for_each over 2-bit packed runs (call site src/fastxsketch.cpp:416-417).
#pragma once
#include "d2g_internal.h"
#include "d2g_plan.h"                 // K1_THREADS, K1_CHUNK, K1_CPT, K1_BLOCK_CHUNKS: the geometry the plan is built for
#include "d2g_minq.h"                 // the windowed walker's sliding minimum
#include <type_traits>

// Thomas Wang's 64-bit mix (sketch::hash::WangHash::hash; call sites src/enums.h:138, src/oph.h:49)
__device__ __forceinline__ uint64_t wang64(uint64_t k) {
    k = ~k + (k << 21);
    k ^= k >> 24;
    k = k + (k << 3) + (k << 8);
    k ^= k >> 14;
    k = k + (k << 2) + (k << 4);
    k ^= k >> 28;
    k += k << 31;
    return k;
}

// launch plan of one batch of genomes: 64-k-mer chunks per run, <= K1_BLOCK_CHUNKS chunks of ONE
// genome per workgroup (built on the host by d2g_plan_build, d2g_plan.cpp)
struct KmerArgs {
    const uint32_t *packed;        // 16 bases per dword, base p at bits [2(p%16), +2)
    const uint64_t *run_start;
    const uint32_t *run_len;
    const uint64_t *run_chunk_off; // [nrun+1] exclusive prefix of chunks per run
    const uint32_t *blk_genome;
    const uint64_t *blk_chunk0;
    const uint32_t *blk_nchunks;
    const uint32_t *blk_run_lo;
    const uint32_t *blk_run_hi;
    int k;
    // K1a, a protein alphabet: an amino-acid k-mer has no canonical form, so the alphabet's size A (6, 8, 14 or 20) stands where
    // canon does -- read under this name only by the AA instantiations of the walker below; a DNA batch holds 0 or 1 here and every
    // field is where it was.  The HOST only ever writes and reads `canon` (d2g_plan_kmer_args, d2g_k1.h, stores 0 / 1 for DNA and A for
    // a protein alphabet; d2g_km_protein() below tells them apart by canon > 1); `asize` is read on the device alone, from the byte copy
    // of the struct that a kernel launch makes -- no member is read on the side that wrote the other.
    union { int canon; uint32_t asize; };
    uint32_t blk0;                 // first launch-plan block of this launch (a launch may cover a sub-range of the plan)
    // K1w, -w > k: k-mers per window, q = w - k + 1 (1 = no window).  Read only by the WIN instantiations of the walker below; it sits
    // in what was padding in front of ftab, so every other field is where it was.
    uint32_t q;
    // K1f, --filterset (d2g_filter.hip): open-addressing table of RAW (canonical when canon) k-mers; nullptr = no filter.
    // Read only by the FILT instantiations of the walker below.
    const uint64_t *ftab;          // [fmask + 1] keys, D2G_FILTER_EMPTY = free slot; [fmask + 1] != 0: the all-ones k-mer is in the set
    uint32_t fmask;                // slots - 1 (a power of two, >= twice the k-mers put in: the probe always ends)
    uint32_t fshift;               // 64 - log2(slots)
};

inline bool d2g_km_protein(const KmerArgs &a) { return a.canon > 1; }
// The walker instantiation a batch takes: f(FILT, WIN, AA) with three std::bool_constants -- a filter attached, minimizers of a
// window, a protein alphabet -- over exactly the six combinations that exist (K1a: never a window with a protein alphabet).  Every
// pass over one batch chooses through this, so all of them drop and walk the same k-mers.
template <class F> auto d2g_walker_variant(const KmerArgs &a, F &&f) {
    constexpr std::true_type Y{}; constexpr std::false_type N{};
    const bool filt = a.ftab != nullptr;
    if (d2g_km_protein(a)) return filt ? f(Y, N, Y) : f(N, N, Y);
    if (a.q > 1) return filt ? f(Y, Y, N) : f(N, Y, N);
    return filt ? f(Y, N, N) : f(N, N, N);
}

// the all-ones k-mer (T x 32, forward) is a legal key and the value of a free slot: its membership is a flag behind the table
constexpr uint64_t D2G_FILTER_EMPTY = ~0ull;
__device__ __forceinline__ uint32_t d2g_filter_slot(uint64_t x, uint32_t shift) { return (uint32_t)((x * 0x9E3779B97F4A7C15ull) >> shift); }
// is k-mer x in the table?  v = the key at x's home slot, loaded by the caller (sixteen independent loads in front of sixteen answers)
__device__ __forceinline__ bool d2g_filter_hit(const KmerArgs &a, uint64_t x, uint64_t v) {
    if (x == D2G_FILTER_EMPTY) return a.ftab[(size_t)a.fmask + 1] != 0;
    uint32_t s = d2g_filter_slot(x, a.fshift);
    while (v != x && v != D2G_FILTER_EMPTY) { s = (s + 1) & a.fmask; v = a.ftab[s]; }
    return v == x;
}
// K1s (d2g_screen.hip): the same probe, answering WHERE x sits -- its slot, fmask + 1 for the all-ones k-mer (held behind the slots),
// D2G_FILTER_NOSLOT when x is not in the table.  Both special values are real slot numbers of a table of 2^32 slots: a table asked
// through this has at most 2^31 (d2g_screen_table_slots refuses more), so fmask + 1 <= 2^31 neither wraps nor meets ~0.
constexpr uint32_t D2G_FILTER_NOSLOT = ~0u;
__device__ __forceinline__ uint32_t d2g_filter_find(const KmerArgs &a, uint64_t x, uint64_t v) {
    if (x == D2G_FILTER_EMPTY) return a.ftab[(size_t)a.fmask + 1] != 0 ? a.fmask + 1 : D2G_FILTER_NOSLOT;
    uint32_t s = d2g_filter_slot(x, a.fshift);
    while (v != x && v != D2G_FILTER_EMPTY) { s = (s + 1) & a.fmask; v = a.ftab[s]; }
    return v == x ? s : D2G_FILTER_NOSLOT;
}

// funnel shift: low 32 bits of (hi:lo) >> sh, 0 <= sh < 32
__device__ __forceinline__ uint32_t fsr(uint32_t hi, uint32_t lo, uint32_t sh) {
    return __builtin_amdgcn_alignbit(hi, lo, sh);
}

// K1w: the windowed walker, -w > k (the reference's bns::Encoder with a Spacer(k, w) and score::Lex; restated from its published
// form, parity unpinned).  A chunk is K1_CHUNK consecutive WINDOW POSITIONS of one run; position i emits the k-mer of x_i .. x_{i+q-1}
// with the smallest score x ^ D2G_LEX_XOR, once per position.  The lane rolls q - 1 k-mers ahead of its first position and keeps the
// window's minimum in a register queue (d2g_minq.h).  The emitted k-mer then meets the filter / the screen's table as any k-mer does.
// Reads: only dwords that hold a base of the lane's own positions' windows, all inside the run -- nothing the tail pad has to cover.
constexpr int D2G_MINQ_DEPTH = 8;

struct D2gBaseStream {            // the packed bases from base index p on, one at a time; a dword is loaded when its first base is asked for
    const uint32_t *w; uint32_t W; int have;
    __device__ __forceinline__ D2gBaseStream(const uint32_t *packed, uint64_t p) : w(packed + (p >> 4)) {
        const uint32_t o = (uint32_t)(p & 15);
        W = *w >> (2 * o); have = 16 - (int)o;
    }
    __device__ __forceinline__ uint64_t next() {
        if (have == 0) { W = *++w; have = 16; }
        const uint64_t cb = W & 3u;
        W >>= 2; --have;
        return cb;
    }
};

template <bool FILT, bool HITS, class F>
__device__ __forceinline__ void d2g_for_each_minimizer_its(const KmerArgs &a, int it0, int it1, F &&f) {
    const int tid = threadIdx.x;
    const uint32_t b = blockIdx.x + a.blk0;
    const uint64_t c0 = a.blk_chunk0[b];
    const uint32_t nc = a.blk_nchunks[b];
    const uint32_t rlo = a.blk_run_lo[b], rhi = a.blk_run_hi[b];
    const int k = a.k, q = (int)a.q;
    const uint64_t kmask = k == 32 ? ~0ull : ((1ull << (2 * k)) - 1);
    const int rcshift = 2 * (k - 1);
    const bool canon = a.canon != 0;

    for (int it = it0; it < it1; ++it) {
        const uint32_t ci_blk = it * K1_THREADS + tid;
        if (ci_blk >= nc) break;
        const uint64_t c = c0 + ci_blk;
        // run containing chunk c: the LAST run of the block that starts at or before it (a run shorter than w owns no chunk)
        uint32_t lo = rlo, hi = rhi;
        while (hi - lo > 1) {
            const uint32_t mid = (lo + hi) >> 1;
            if (a.run_chunk_off[mid] <= c) lo = mid; else hi = mid;
        }
        const uint64_t ci = c - a.run_chunk_off[lo];
        const uint64_t np = (uint64_t)a.run_len[lo] - (uint32_t)(k + q - 1) + 1;    // window positions of the run (len >= w: it owns a chunk)
        const uint64_t p = a.run_start[lo] + ci * K1_CHUNK;                         // first base of the lane's first window
        const uint64_t left = np - ci * K1_CHUNK;
        const int n = left < (uint64_t)K1_CHUNK ? (int)left : K1_CHUNK;

        D2gBaseStream bs(a.packed, p);
        uint64_t fwd = 0, rc = 0;
        for (int j = 0; j < k - 1; ++j) {
            const uint64_t cb = bs.next();
            fwd = (fwd << 2) | cb;
            rc = (rc >> 2) | ((3 - cb) << rcshift);
        }
        D2gMinQueue<D2G_MINQ_DEPTH> mq;
        mq.clear();
        const int steps = q - 1 + n;                                                // k-mers t = 0 .. q - 2 + n; position i closes at t = i + q - 1
#pragma unroll 1
        for (int t = 0; t < steps; ++t) {
            const uint64_t cb = bs.next();
            fwd = ((fwd << 2) | cb) & kmask;
            rc = (rc >> 2) | ((3 - cb) << rcshift);
            mq.push((canon ? (fwd < rc ? fwd : rc) : fwd) ^ D2G_LEX_XOR, t);
            const int first = t - (q - 1);
            if (first < 0) continue;
            mq.expire(first);
            if (mq.empty()) {
                // every entry the queue kept has left and later ones were dropped: the window's q k-mers once more
                D2gBaseStream rs(a.packed, p + (uint64_t)first);
                uint64_t f2 = 0, r2 = 0;
                for (int j = 0; j < k - 1; ++j) {
                    const uint64_t c2 = rs.next();
                    f2 = (f2 << 2) | c2;
                    r2 = (r2 >> 2) | ((3 - c2) << rcshift);
                }
                mq.clear();
#pragma unroll 1
                for (int u = first; u <= t; ++u) {
                    const uint64_t c2 = rs.next();
                    f2 = ((f2 << 2) | c2) & kmask;
                    r2 = (r2 >> 2) | ((3 - c2) << rcshift);
                    mq.push((canon ? (f2 < r2 ? f2 : r2) : f2) ^ D2G_LEX_XOR, u);
                }
            }
            const uint64_t x = mq.front() ^ D2G_LEX_XOR;
            if constexpr (FILT) {
                const uint64_t v = a.ftab[d2g_filter_slot(x, a.fshift)];
                if constexpr (HITS) {
                    const uint32_t slot = d2g_filter_find(a, x, v);
                    if (slot != D2G_FILTER_NOSLOT) f(x, slot);
                } else {
                    if (!d2g_filter_hit(a, x, v)) f(x);
                }
            } else {
                f(x);
            }
        }
    }
}

// K1a: the amino-acid walker (spec D2G-AA; the reference's bns::Encoder over a protein alphabet, restated: parity
// unpinned).  The stream holds ONE BYTE per residue, its code c < A; the key of residues c_0 .. c_{k-1} is sum c_j A^(k-1-j), below
// A^k <= 2^64.  A chunk is K1_CHUNK consecutive k-mer starts of one run, as for DNA.  The lane keeps y = the value of the k - 1
// residues in front of the next one; a step is
//     x = y * A + in          the k-mer that ends at `in` (y < A^(k-1), so x < A^k: nothing wraps)
//     y = x - out * A^(k-1)   its first residue `out` leaves
// `in` (residue p + k - 1 + e) and `out` (residue p + e) come from two windows of sixteen bytes, each five dwords aligned to the run's
// byte offset with alignbit; a run starts at any byte of a dword.  A and A^(k-1) are run-time values, uniform over the launch.
// Reads: the bytes of the lane's own k-mers and at most 19 bytes behind the run's last one (the stream's 64-byte pad covers them).
// FILT as for DNA: sixteen k-mers, then sixteen home-slot loads in flight.  There is no canonical form, no HITS and no WIN.
template <bool FILT, class F>
__device__ __forceinline__ void d2g_for_each_aa_kmer_its(const KmerArgs &a, int it0, int it1, F &&f) {
    const int tid = threadIdx.x;
    const uint32_t b = blockIdx.x + a.blk0;
    const uint64_t c0 = a.blk_chunk0[b];
    const uint32_t nc = a.blk_nchunks[b];
    const uint32_t rlo = a.blk_run_lo[b], rhi = a.blk_run_hi[b];
    const int k = a.k;
    const uint64_t A = a.asize;
    uint64_t apow = 1;
    for (int j = 1; j < k; ++j) apow *= A;

    for (int it = it0; it < it1; ++it) {
        const uint32_t ci_blk = it * K1_THREADS + tid;
        if (ci_blk >= nc) break;
        const uint64_t c = c0 + ci_blk;
        uint32_t lo = rlo, hi = rhi;
        while (hi - lo > 1) {
            const uint32_t mid = (lo + hi) >> 1;
            if (a.run_chunk_off[mid] <= c) lo = mid; else hi = mid;
        }
        const uint64_t ci = c - a.run_chunk_off[lo];
        const uint64_t nk = (uint64_t)a.run_len[lo] - k + 1;
        const uint64_t p = a.run_start[lo] + ci * K1_CHUNK;       // first k-mer start (residue = byte index)
        const uint64_t left = nk - ci * K1_CHUNK;
        const int n = left < (uint64_t)K1_CHUNK ? (int)left : K1_CHUNK;

        const uint32_t *wo = a.packed + (p >> 2);                 // the window that leaves: residues [p, p + 64)
        const uint32_t sho = (uint32_t)(p & 3) * 8;
        // warm-up: residues [p, p + k - 1), at most 23: whole dwords of four, then the one to three that are left.  Two short
        // loops with uniform trip counts and not an unrolled, predicated ladder: that kept 24 conditions alive in SGPRs
        uint64_t y = 0;
        {
            const int full = (k - 1) >> 2, rest = (k - 1) & 3;
            uint32_t wprev = wo[0];
#pragma unroll 1
            for (int g = 0; g < full; ++g) {
                const uint32_t wnext = wo[g + 1];
                const uint32_t W = fsr(wnext, wprev, sho);
                wprev = wnext;
#pragma unroll
                for (int e = 0; e < 4; ++e) y = y * A + ((W >> (8 * e)) & 0xffu);
            }
            if (rest) {
                uint32_t W = fsr(wo[full + 1], wprev, sho);
#pragma unroll 1
                for (int e = 0; e < rest; ++e) { y = y * A + (W & 0xffu); W >>= 8; }
            }
        }
        const uint64_t q = p + (uint64_t)(k - 1);                 // the window that enters: residues [q, q + 64)
        const uint32_t *wn = a.packed + (q >> 2);
        const uint32_t shn = (uint32_t)(q & 3) * 8;
#pragma unroll 1
        for (int wi = 0; wi < 4; ++wi) {
            const int ebase = wi * 16;
            if (ebase >= n) break;
            uint32_t I[4], O[4];
            {
                const uint32_t *w = wn + 4 * wi;
                const uint32_t w0 = w[0], w1 = w[1], w2 = w[2], w3 = w[3], w4 = w[4];
                I[0] = fsr(w1, w0, shn); I[1] = fsr(w2, w1, shn); I[2] = fsr(w3, w2, shn); I[3] = fsr(w4, w3, shn);
            }
            {
                const uint32_t *w = wo + 4 * wi;
                const uint32_t w0 = w[0], w1 = w[1], w2 = w[2], w3 = w[3], w4 = w[4];
                O[0] = fsr(w1, w0, sho); O[1] = fsr(w2, w1, sho); O[2] = fsr(w3, w2, sho); O[3] = fsr(w4, w3, sho);
            }
            if constexpr (FILT) {
                uint64_t xs[16], vs[16];
#pragma unroll
                for (int e = 0; e < 16; ++e) {
                    const uint64_t x = y * A + ((I[e >> 2] >> (8 * (e & 3))) & 0xffu);
                    y = x - (uint64_t)((O[e >> 2] >> (8 * (e & 3))) & 0xffu) * apow;
                    xs[e] = x;
                    vs[e] = ebase + e < n ? a.ftab[d2g_filter_slot(x, a.fshift)] : 0;
                }
#pragma unroll
                for (int e = 0; e < 16; ++e)
                    if (ebase + e < n && !d2g_filter_hit(a, xs[e], vs[e])) f(xs[e]);
                continue;
            }
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const uint64_t x = y * A + ((I[e >> 2] >> (8 * (e & 3))) & 0xffu);
                y = x - (uint64_t)((O[e >> 2] >> (8 * (e & 3))) & 0xffu) * apow;
                if (ebase + e < n) f(x);
            }
        }
    }
}

// f(x) once per k-mer of the chunks this lane owns in workgroup blockIdx.x; x = canonical
// (min(fwd, revcomp)) or forward 2-bit k-mer.  A lane owns chunk (it * K1_THREADS + tid).
// IT0 <= it < IT1: the passes ("tiles" of K1_THREADS chunks = K1_THREADS * K1_CHUNK k-mers) of the workgroup to walk
// FILT: f sees only the k-mers that are NOT in a.ftab (the reference's `!opts.fs_->in_set(maskfn(x))`, src/fastxsketch.cpp:387) --
// a template flag, so that the unfiltered instantiations are the code they were (profiles/filter_resource_usage.txt)
// HITS (with FILT): the third mode, K1s -- f(x, slot) for the k-mers that ARE in a.ftab, slot as d2g_filter_find gives it; a miss
// does nothing.  The other instantiations stay the code they were (profiles/screen_resource_usage.txt)
// WIN: the fourth, K1w -- f sees the minimizer of every window position instead (d2g_for_each_minimizer_its above), under either of
// the other two flags.  The unwindowed instantiations stay the code they were (profiles/window_resource_usage.txt)
// AA: the fifth, K1a -- f sees the amino-acid k-mers of a byte-per-residue stream (d2g_for_each_aa_kmer_its above), under FILT or
// not.  The DNA instantiations stay the code they were (profiles/protein_resource_usage.txt)
template <bool FILT = false, bool HITS = false, bool WIN = false, bool AA = false, class F>
__device__ __forceinline__ void d2g_for_each_kmer_its(const KmerArgs &a, int it0, int it1, F &&f) {
    if constexpr (AA) {
        static_assert(!HITS && !WIN, "the amino-acid walker knows neither the hit mode nor a window");
        d2g_for_each_aa_kmer_its<FILT>(a, it0, it1, static_cast<F &&>(f));
        return;
    }
    if constexpr (WIN) {
        d2g_for_each_minimizer_its<FILT, HITS>(a, it0, it1, static_cast<F &&>(f));
        return;
    }
    const int tid = threadIdx.x;
    const uint32_t b = blockIdx.x + a.blk0;
    const uint64_t c0 = a.blk_chunk0[b];
    const uint32_t nc = a.blk_nchunks[b];
    const uint32_t rlo = a.blk_run_lo[b], rhi = a.blk_run_hi[b];
    const int k = a.k;
    const uint64_t kmask = k == 32 ? ~0ull : ((1ull << (2 * k)) - 1);
    const int rcshift = 2 * (k - 1);
    const bool canon = a.canon != 0;

    for (int it = it0; it < it1; ++it) {
        const uint32_t ci_blk = it * K1_THREADS + tid;
        if (ci_blk >= nc) break;
        const uint64_t c = c0 + ci_blk;
        // run containing chunk c (runs of this block only: usually a single candidate)
        uint32_t lo = rlo, hi = rhi;
        while (hi - lo > 1) {
            const uint32_t mid = (lo + hi) >> 1;
            if (a.run_chunk_off[mid] <= c) lo = mid; else hi = mid;
        }
        const uint64_t ci = c - a.run_chunk_off[lo];
        const uint64_t nk = (uint64_t)a.run_len[lo] - k + 1;
        const uint64_t p = a.run_start[lo] + ci * K1_CHUNK;       // first k-mer start (base index)
        const uint64_t left = nk - ci * K1_CHUNK;
        const int n = left < (uint64_t)K1_CHUNK ? (int)left : K1_CHUNK;

        // warm-up window: bases [p, p+k-1) (<= 31 bases) as one 64-bit value
        uint64_t fwd = 0, rc = 0;
        {
            const uint32_t *w = a.packed + (p >> 4);
            const uint32_t sh = (uint32_t)(p & 15) * 2;
            const uint32_t w0 = w[0], w1 = w[1], w2 = w[2];
            uint64_t X = ((uint64_t)fsr(w2, w1, sh) << 32) | fsr(w1, w0, sh);
            for (int j = 0; j < k - 1; ++j) {
                const uint64_t cb = X & 3;
                X >>= 2;
                fwd = (fwd << 2) | cb;
                rc = (rc >> 2) | ((3 - cb) << rcshift);
            }
        }
        // main window: bases [q, q+64), q = p + k - 1, aligned into 4 dwords
        uint32_t M0, M1, M2, M3;
        {
            const uint64_t q = p + (uint64_t)(k - 1);
            const uint32_t *w = a.packed + (q >> 4);
            const uint32_t sh = (uint32_t)(q & 15) * 2;
            const uint32_t w0 = w[0], w1 = w[1], w2 = w[2], w3 = w[3], w4 = w[4];
            M0 = fsr(w1, w0, sh); M1 = fsr(w2, w1, sh); M2 = fsr(w3, w2, sh); M3 = fsr(w4, w3, sh);
        }
#pragma unroll 1
        for (int wi = 0; wi < 4; ++wi) {
            const uint32_t W = wi == 0 ? M0 : wi == 1 ? M1 : wi == 2 ? M2 : M3;
            const int ebase = wi * 16;
            if (ebase >= n) break;
            if constexpr (FILT) {
                // the sixteen k-mers of the word first, each with the load of its home slot: sixteen random reads in flight
                // instead of one dependent round trip per k-mer
                uint64_t xs[16], vs[16];
#pragma unroll
                for (int e = 0; e < 16; ++e) {
                    const uint64_t cb = (W >> (2 * e)) & 3u;
                    fwd = ((fwd << 2) | cb) & kmask;
                    rc = (rc >> 2) | ((3 - cb) << rcshift);
                    xs[e] = canon ? (fwd < rc ? fwd : rc) : fwd;
                    vs[e] = ebase + e < n ? a.ftab[d2g_filter_slot(xs[e], a.fshift)] : 0;
                }
                if constexpr (HITS) {
#pragma unroll
                    for (int e = 0; e < 16; ++e)
                        if (ebase + e < n) {
                            const uint32_t slot = d2g_filter_find(a, xs[e], vs[e]);
                            if (slot != D2G_FILTER_NOSLOT) f(xs[e], slot);
                        }
                } else {
#pragma unroll
                    for (int e = 0; e < 16; ++e)
                        if (ebase + e < n && !d2g_filter_hit(a, xs[e], vs[e])) f(xs[e]);
                }
                continue;
            }
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const uint64_t cb = (W >> (2 * e)) & 3u;
                fwd = ((fwd << 2) | cb) & kmask;
                rc = (rc >> 2) | ((3 - cb) << rcshift);
                if constexpr (!HITS)                             // (the hit mode left through the FILT arm; its f takes two arguments)
                    if (ebase + e < n) f(canon ? (fwd < rc ? fwd : rc) : fwd);
            }
        }
    }
}

template <bool FILT = false, bool HITS = false, bool WIN = false, bool AA = false, class F>
__device__ __forceinline__ void d2g_for_each_kmer(const KmerArgs &a, F &&f) {
    static_assert(FILT || !HITS, "the hit mode walks a table");
    d2g_for_each_kmer_its<FILT, HITS, WIN, AA>(a, 0, K1_CPT, static_cast<F &&>(f));
}
