// d2g_k3_bmh.hip -- K3: the --multiset sketch path on gfx950.
//
//   R11  exact k-mer counting      reference src/counter.h:68-77 (Counter::add(uint64_t)), finalize 118-138,
//                                  driver src/fastxsketch.cpp:425-445
//   R12  BagMinHash                sketch::BagMinHash2<double> (ABSENT dnbaker/sketch bmh.h; parity unpinned);
//                                  restated from Ertl, KDD 2018 under the "BMH-D2G" spec of DESIGN.md
//
// The reference counts with one robin-hood hash map per thread and feeds (kmer, count) to the
// sketch one at a time.  Here (this unit holds step 2, K3o and K3Run::run; the other families of K3 and what they share: d2g_k3.h):
//   1. k3_hist / k3_scan / k3_scatter / k3_refine (d2g_k3_bucket.hip) : every masked k-mer key = Wang(kmer ^ XORMASK) of a genome is
//      multi-split by its top bits into <= 4096 buckets of ~1-2 K keys (LDS-aggregated histogram, one global
//      reservation per (workgroup, write front)), in two levels so that a workgroup keeps <= 256 write fronts open
//      and the L2 completes the lines (see k3_scatter_kernel); k-mers are re-generated from the packed bases in
//      each enumerating pass instead of being stored (generation is ~100 VALU slots, a store+load is 16 B).
//   2. k3_bmh_main / k3_bmh_survivor / k3_bmh_verify : persistent workgroups walk the buckets; each bucket is counted
//      exactly in a 2048-slot LDS open-addressing table (ds_cmpst_b64 claim + ds_add), then every occupied
//      slot IS one (key, count) element: the first point of each of its top-level strips is tested against a bound
//      of the genome's final maximum register (99 % stop there), the survivors are queued -- in HBM, walked by the
//      survivor kernel one per lane (first pass), or in LDS and drained in place (repeat passes) -- and the
//      BagMinHash Poisson-process tree is walked for them depth-first with a private stack.
//      Registers live in HBM/L2 as the bit patterns of non-negative doubles and are lowered with
//      global_atomic_umin_x2 behind a read filter.
//      min is order-free and pruning by ANY bound >= the final maximum only drops points that cannot win,
//      so the result is bit-identical to the time-ordered sequential algorithm (oracle/d2_bmh_oracle.c).
//      The bound is GUESSED from the genome's total weight (max of m exponentials of rate W/m) and
//      VERIFIED afterwards (max(h) <= guess); a genome that fails is walked again under a 16x larger
//      guess (idempotent: registers only go down).
#include "d2g_k3_device.h"
#include <algorithm>
#include <cmath>
#include <cstring>

namespace {

constexpr int K3_TAB = 2048;                // LDS count-table slots (24.6 KB with the counts: 6 workgroups per CU)
constexpr uint64_t BMH_INF = 0x7FF0000000000000ull;

// ---------------------------------------------------------------------------------------------
// exact counting of one bucket round into the LDS table
// ---------------------------------------------------------------------------------------------
// key type of the main-side code: the 64-bit masked key (generic path) or the 32-bit stored word (compact path)
template <bool C32> struct K3Key;
template <> struct K3Key<false> {
    typedef uint64_t T;
    static constexpr uint64_t EMPTY = ~0ull;
    // the key IS a hash (Wang of the masked k-mer): bits 32..42 are as good as any product of it, and are not the ones that
    // chose the bucket (top 12), the sub-range or the round (low bits)
    static __device__ __forceinline__ uint32_t slot(uint64_t key) { return (uint32_t)(key >> 32) & (K3_TAB - 1); }
    // R rounds: key bits [shift, shift + log2 R) (the bits below `shift` chose the sub-range)
    static __device__ __forceinline__ uint32_t round_of(uint64_t key, uint32_t R, uint32_t shift, uint32_t) { return (uint32_t)(key >> shift) & (R - 1); }
    static __device__ __forceinline__ uint32_t sub_of(uint64_t key, uint32_t R, uint32_t) { return (uint32_t)key & (R - 1); }
};
template <> struct K3Key<true> {
    typedef uint32_t T;
    static constexpr uint32_t EMPTY = ~0u;
    static __device__ __forceinline__ uint32_t slot(uint32_t lo) { return (lo * 0x85EBCA6Bu) >> 21; }
    // bits of m = lo * K3C_MUL from the top: bb bucket bits, then `shift` sub-range bits, then log2 R round bits
    static __device__ __forceinline__ uint32_t round_of(uint32_t lo, uint32_t R, uint32_t shift, uint32_t bb) {
        const uint32_t v = (k3c_mix(lo) << bb) << shift;            // bb + shift + log2 R <= 32 (checked on the host)
        return R > 1 ? v >> (__clz(R) + 1) : 0u;                     // 32 - log2 R = clz(R) + 1
    }
    static __device__ __forceinline__ uint32_t sub_of(uint32_t lo, uint32_t R, uint32_t bb) {
        return R > 1 ? (k3c_mix(lo) << bb) >> (__clz(R) + 1) : 0u;
    }
};
static_assert(K3_TAB == 1 << 11, "the slot hashes take the top 11 bits");

template <bool C32>
struct CountTab {
    typename K3Key<C32>::T *key;   // [K3_TAB]
    uint32_t *cnt;                 // [K3_TAB]
    uint32_t *ones;                // count of the key == EMPTY (cannot live in the table)
};

// keys of round r of R (R a power of two) of one key range; returns false on overflow
template <bool C32>
__device__ bool count_round(const CountTab<C32> &t, const typename K3Key<C32>::T *kb, uint64_t n, uint32_t R, uint32_t r, uint32_t shift,
                            uint32_t bb) {
    typedef typename K3Key<C32>::T KT;
    constexpr KT EMPTY = K3Key<C32>::EMPTY;
    const int tid = threadIdx.x;
    for (int s = tid; s < K3_TAB; s += K3_THREADS) { t.key[s] = EMPTY; t.cnt[s] = 0; }
    if (tid == 0) *t.ones = 0;
    __syncthreads();
    bool ok = true;
    // keys are fetched K3_KPF per lane at a time BEFORE the probe chains: with the load inside the
    // probing loop every key exposed a full HBM/L2 round trip (measured 25 us per 1220-key bucket)
    constexpr int K3_KPF = C32 ? 8 : 6;
    for (uint64_t base = 0; base < n && ok; base += (uint64_t)K3_KPF * K3_THREADS) {
        KT kreg[K3_KPF];
#pragma unroll
        for (int j = 0; j < K3_KPF; ++j) {
            const uint64_t i = base + (uint64_t)j * K3_THREADS + tid;
            kreg[j] = i < n ? kb[i] : 0;
        }
#pragma unroll
        for (int j = 0; j < K3_KPF; ++j) {
            const uint64_t i = base + (uint64_t)j * K3_THREADS + tid;
            const KT key = kreg[j];
            const bool mine = i < n && (R == 1 || K3Key<C32>::round_of(key, R, shift, bb) == r);
            if (mine && key == EMPTY) atomicAdd(t.ones, 1u);
            if (!mine || key == EMPTY) continue;
            // one exit test per probe (structured-control-flow bookkeeping is SALU work: the first
            // version of this loop issued 30 scalar instructions per probe)
            uint32_t s = K3Key<C32>::slot(key);
            int probes = 0;
            bool placed;
            for (;;) {
                KT cur = t.key[s];
                if (cur == EMPTY) {
                    if constexpr (C32) cur = atomicCAS(&t.key[s], EMPTY, key) == EMPTY ? key : t.key[s];
                    else cur = atomicCAS((unsigned long long *)&t.key[s], (unsigned long long)EMPTY, (unsigned long long)key) == EMPTY ? key : t.key[s];
                }
                placed = cur == key;
                if (placed | (++probes >= K3_TAB)) break;
                s = (s + 1) & (K3_TAB - 1);
            }
            if (placed) atomicAdd(&t.cnt[s], 1u); else ok = false;
        }
    }
    const bool res = !__syncthreads_or(!ok);
    return res;
}

// The main kernel's round: the table arrives CLEAN (the walk that follows each round empties the slots it reads), so a
// round is insert -> barrier -> walk+clear -> barrier.  Probing goes compare-and-swap first: one LDS operation and two
// compares per probe (the read-first loop of count_round spends twice the vector instructions; the kernel is bound by
// instruction issue, not by the LDS atomic rate: profiles/r02_k3_ablation.txt).
// GUARD = false (single-round ranges: n <= round_keys < K3_TAB keys, the table cannot fill): the probe loop carries no
// probe counter -- its bookkeeping was 13 scalar instructions per probe next to 6 vector ones.
template <bool C32, bool GUARD>
__device__ bool insert_round(const CountTab<C32> &t, const typename K3Key<C32>::T *kb, uint64_t n, uint32_t R, uint32_t r, uint32_t shift,
                             uint32_t bb) {
    typedef typename K3Key<C32>::T KT;
    constexpr KT EMPTY = K3Key<C32>::EMPTY;
    const int tid = threadIdx.x;
    bool ok = true;
    constexpr int K3_KPF = 6;
    for (uint64_t base = 0; base < n && ok; base += (uint64_t)K3_KPF * K3_THREADS) {
        KT kreg[K3_KPF];
#pragma unroll
        for (int j = 0; j < K3_KPF; ++j) {
            const uint64_t i = base + (uint64_t)j * K3_THREADS + tid;
            kreg[j] = i < n ? kb[i] : 0;
        }
        uint32_t n_ones = 0;                                              // the all-ones key cannot live in the table (rare: one branch per batch)
#pragma unroll
        for (int j = 0; j < K3_KPF; ++j) {
            const uint64_t i = base + (uint64_t)j * K3_THREADS + tid;
            const KT key = kreg[j];
            const bool mine = i < n && (R == 1 || K3Key<C32>::round_of(key, R, shift, bb) == r);
            n_ones += mine & (key == EMPTY);
            if (!mine || key == EMPTY) continue;
            uint32_t s = K3Key<C32>::slot(key);
            if constexpr (GUARD) {
                int probes = 0;
                bool placed;
                for (;;) {
                    KT old;
                    if constexpr (C32) old = atomicCAS(&t.key[s], EMPTY, key);
                    else old = (KT)atomicCAS((unsigned long long *)&t.key[s], (unsigned long long)EMPTY, (unsigned long long)key);
                    placed = (old == EMPTY) | (old == key);
                    if (placed | (++probes >= K3_TAB)) break;
                    s = (s + 1) & (K3_TAB - 1);
                }
                if (placed) atomicAdd(&t.cnt[s], 1u); else ok = false;
            } else {
                for (;;) {
                    KT old;
                    if constexpr (C32) old = atomicCAS(&t.key[s], EMPTY, key);
                    else old = (KT)atomicCAS((unsigned long long *)&t.key[s], (unsigned long long)EMPTY, (unsigned long long)key);
                    if ((old == EMPTY) | (old == key)) break;
                    s = (s + 1) & (K3_TAB - 1);
                }
                atomicAdd(&t.cnt[s], 1u);
            }
        }
        if (n_ones) atomicAdd(t.ones, n_ones);
    }
    if constexpr (GUARD) return !__syncthreads_or(!ok);
    __syncthreads();
    return true;
}

// After count_round: squeeze the occupied slots that pass the count threshold to the front of the
// table arrays (the all-ones key, which cannot live in the table, is appended), so that the walk
// below runs over a dense element list with every lane busy.  Returns the number of elements.
template <bool C32>
__device__ uint32_t compact_elements(const CountTab<C32> &t, uint32_t *nelem, double thr) {
    constexpr int PER = K3_TAB / K3_THREADS;
    const int tid = threadIdx.x;
    typename K3Key<C32>::T k[PER];
    uint32_t c[PER];
    uint32_t mine = 0;
#pragma unroll
    for (int j = 0; j < PER; ++j) {
        const int s = tid + j * K3_THREADS;
        const uint32_t cc = t.cnt[s];
        k[j] = t.key[s];
        c[j] = (cc && (double)cc > thr) ? cc : 0u;                   // counter.h:123: pair.second > threshold
        mine += c[j] != 0;
    }
    const uint32_t ones = *t.ones;
    const bool extra = tid == 0 && ones && (double)ones > thr;
    mine += extra;
    if (tid == 0) *nelem = 0;
    __syncthreads();
    uint32_t pos = mine ? atomicAdd(nelem, mine) : 0u;
    __syncthreads();
#pragma unroll
    for (int j = 0; j < PER; ++j)
        if (c[j]) { t.key[pos] = k[j]; t.cnt[pos] = c[j]; ++pos; }
    if (extra) { t.key[pos] = K3Key<C32>::EMPTY; t.cnt[pos] = ones; }
    __syncthreads();
    return *nelem;
}

// The main pass splits the walk in two.  Phase 1 (every element, every lane): the first point of
// each relevant top strip; 99% die in the early-out of proc_next.  A survivor needs the ~60-level
// descent of bmh_locate, which one lane would run alone while 63 wait -- so survivors are queued in
// LDS and phase 2 drains the queue with one survivor per lane once enough have accumulated.
struct QEntry { uint64_t d; double w; uint32_t t, g; };     // strip t of element (d, w) of genome g: the survivor's
                                                             // process is regenerated in phase 2 (24 B instead of 56)
constexpr int K3_QCAP = 256;
constexpr int K3_QDRAIN = 160;          // drain when at least this many are waiting

struct BmhArgs {
    const uint64_t *keys;        // generic path: bucketed 64-bit masked keys
    const uint32_t *keys32;      // compact path: bucketed 32-bit stored words (k3c_*)
    const uint32_t *g_bbits;     // compact path: [n] bucket bits of genome g
    uint32_t hb;                 // compact path: hi bits = max(0, d2g_key_bits(k, alphabet) - 32): 2k - 32 for DNA
    uint64_t xormask;            // compact path: the masked key Wang(x ^ xormask) is formed per distinct k-mer here
    const uint64_t *bucket_off;
    const uint32_t *g_boff;
    uint32_t n;              // genomes
    uint32_t TB;
    uint32_t m;
    double thr;
    uint64_t *h;             // [n][m] register bit patterns, +inf initially
    uint64_t *guess;         // [n] pruning bound of the current pass (bit pattern of a double)
    double *tw;              // [n] total weight
    uint64_t *tw_acc;        // [n] sum of the counted weights of the first pass (integers; zeroed by the host)
    uint32_t *redo;          // [n] 1 = the guess proved too small: walk this genome again
    uint32_t *nredo;         // [1]
    int redo_mode;           // 0 = first pass (every genome, weights are summed); 1 = only genomes with redo[g]
    uint32_t round_keys;     // K3_ROUND_KEYS; D2G_K3_ROUND_KEYS lowers it (tests force multi-round buckets on small inputs)
    int *status;
    // big inputs: buckets of a genome with g_split[g] = s > 0 were split once more into 2^s sub-ranges by
    // their low key bits (k3_split_kernel): sub-range j of bucket tb = skeys[sub_off[i] .. sub_off[i+1]),
    // i = g_sub[g] + ((tb - g_boff[g]) << s) + j
    const uint32_t *g_split;  // [n] or nullptr
    const uint64_t *g_sub;    // [n+1]
    uint64_t *sub_off;        // [nsub + 1]
    uint64_t *skeys;          // [total k-mers]
    uint32_t *skeys32;        // compact path
    uint32_t tb0, tb1;        // buckets this launch of the main kernel walks (a sub-batch, or [0, TB))
    uint32_t g0;              // first genome of this launch of the verify kernel
    // first pass, light form: survivors queue in HBM, one region per main workgroup
    QEntry *gq; const uint64_t *gq_off; uint32_t *gq_n;
    // optional R11 output (k3_count_kernel): distinct (key,count) written in place of the bucket
    uint64_t *out_keys; uint32_t *out_counts; uint32_t *bucket_nd;
};

template <bool C32>
struct SharedK3 {
    typename K3Key<C32>::T key[K3_TAB + 1 + C32];      // +1: the all-ones key joins the compacted element list (+1: alignment)
    uint32_t cnt[K3_TAB + 2];
    uint64_t red[8];
    uint32_t ones;
    uint32_t misc;
    uint32_t nelem;
    uint32_t pad;
};

// Buckets of big inputs hold far more keys than one table round takes (a 1 Gbp genome: 2.4e5 keys per
// bucket = 256 rounds, each of which would re-read the whole bucket).  This pass splits such a bucket
// ONCE by its low key bits into 2^s contiguous sub-ranges of ~1000 keys, so that every later round reads
// only its own keys.  One workgroup per bucket at a time; the bucket (<= a few MB) stays in L2 between
// the counting and the scattering read.  (With only 4 sub-ranges -- the compact path's case -- the LDS atomics pile on
// four counters; a ballot/popcount partition without atomics was measured and is no faster, 6.9 vs 6.3 ms per 1.25e9
// keys: the pass is bound by the per-bucket latency chain, not by the counters.)
template <bool C32>
__global__ __launch_bounds__(K3_THREADS) void k3_split_kernel(BmhArgs a) {
    typedef typename K3Key<C32>::T KT;
    __shared__ uint32_t pos[K3_MAXB];
    __shared__ uint32_t wsum[K3_THREADS / 64];
    const uint32_t tid = threadIdx.x;
    for (uint32_t tb = blockIdx.x; tb < a.TB; tb += gridDim.x) {
        const uint32_t g = genome_of_bucket(a.g_boff, a.n, tb);
        const uint32_t sb = a.g_split[g];
        if (sb == 0) continue;
        const uint32_t R = 1u << sb;
        const uint64_t o0 = a.bucket_off[tb], nk = a.bucket_off[tb + 1] - o0;
        const KT *kb = (C32 ? (const KT *)a.keys32 : (const KT *)a.keys) + o0;
        const uint32_t bb = C32 ? a.g_bbits[g] : 0u;
        const uint64_t base = a.g_sub[g] + ((uint64_t)(tb - a.g_boff[g]) << sb);
        for (uint32_t i = tid; i < R; i += K3_THREADS) pos[i] = 0;
        __syncthreads();
        constexpr int PF = 8;
        for (uint64_t b0 = 0; b0 < nk; b0 += (uint64_t)PF * K3_THREADS) {
            KT kk[PF];
#pragma unroll
            for (int j = 0; j < PF; ++j) { const uint64_t i = b0 + (uint64_t)j * K3_THREADS + tid; kk[j] = i < nk ? kb[i] : 0; }
#pragma unroll
            for (int j = 0; j < PF; ++j) if (b0 + (uint64_t)j * K3_THREADS + tid < nk) atomicAdd(&pos[K3Key<C32>::sub_of(kk[j], R, bb)], 1u);
        }
        __syncthreads();
        // exclusive prefix of pos[0..R): each thread owns R / 256 consecutive counters (R <= 4096)
        const uint32_t per = (R + K3_THREADS - 1) / K3_THREADS, lo = min(R, tid * per), hi = min(R, lo + per);
        uint32_t sum = 0;
        for (uint32_t i = lo; i < hi; ++i) sum += pos[i];
        uint32_t incl = sum;
        for (int o = 1; o < 64; o <<= 1) { const uint32_t v = __shfl_up(incl, o); if ((tid & 63) >= (uint32_t)o) incl += v; }
        if ((tid & 63) == 63) wsum[tid >> 6] = incl;
        __syncthreads();
        uint32_t run = incl - sum;
        for (uint32_t w = 0; w < (tid >> 6); ++w) run += wsum[w];
        for (uint32_t i = lo; i < hi; ++i) { const uint32_t c = pos[i]; pos[i] = run; a.sub_off[base + i] = o0 + run; run += c; }
        if (tid == 0) a.sub_off[base + R] = o0 + nk;            // = the next bucket's first entry (same value), or the genome's end
        __syncthreads();
        KT *dst = (C32 ? (KT *)a.skeys32 : (KT *)a.skeys) + o0;
        for (uint64_t b0 = 0; b0 < nk; b0 += (uint64_t)PF * K3_THREADS) {
            KT kk[PF];
#pragma unroll
            for (int j = 0; j < PF; ++j) { const uint64_t i = b0 + (uint64_t)j * K3_THREADS + tid; kk[j] = i < nk ? kb[i] : 0; }
#pragma unroll
            for (int j = 0; j < PF; ++j)
                if (b0 + (uint64_t)j * K3_THREADS + tid < nk) dst[atomicAdd(&pos[K3Key<C32>::sub_of(kk[j], R, bb)], 1u)] = kk[j];
        }
        __syncthreads();
    }
}

// registers to +inf, weights to zero
__global__ __launch_bounds__(K3_THREADS) void k3_bmh_init_kernel(uint64_t *h, size_t nh, double *tw, uint32_t *redo, size_t n) {
    const size_t i = (size_t)blockIdx.x * K3_THREADS + threadIdx.x;
    if (i < nh) h[i] = BMH_INF;
    if (i < n) { tw[i] = 0.; redo[i] = 0; }
}

#ifndef D2G_K3_WPE
#define D2G_K3_WPE 5
#endif
#ifndef D2G_K3_WPE_LIGHT
#define D2G_K3_WPE_LIGHT 6
#endif
// LIGHT (the first pass): survivors are not walked here but appended to the workgroup's region of a queue in HBM and
// walked by k3_bmh_survivor_kernel afterwards, one per lane with every lane busy.  Without the descent (its stack, its
// LDS queue, its drains and their barriers) this kernel needs fewer registers and less LDS: 6 workgroups per CU instead of 5.
// The heavy form stays for the repeat passes (guess too small: rare) and as the fallback when a region overflows.
template <bool C32, bool LIGHT>
__global__ __launch_bounds__(K3_THREADS) __attribute__((amdgpu_waves_per_eu(LIGHT ? D2G_K3_WPE_LIGHT : D2G_K3_WPE))) void k3_bmh_main_kernel(BmhArgs a) {
    typedef typename K3Key<C32>::T KT;
    __shared__ SharedK3<C32> sh;
    __shared__ QEntry queue[LIGHT ? 1 : K3_QCAP];
    __shared__ uint32_t qn;
    const int tid = threadIdx.x;
    const uint32_t m = a.m;
    const CountTab<C32> t{sh.key, sh.cnt, &sh.ones};
    Proc stk[LIGHT ? 1 : BMH_STACK];
    if (tid == 0) qn = 0;
    if (LIGHT && tid == 0) a.gq_n[blockIdx.x] = 0;
    __syncthreads();
    // phase 2: one queued survivor per lane
    auto drain = [&]() {
        if constexpr (LIGHT) return;
        const uint32_t n = qn < (uint32_t)K3_QCAP ? qn : (uint32_t)K3_QCAP;
        for (uint32_t i = tid; i < n; i += K3_THREADS) {
            const QEntry q = queue[i];
            const double bound = V(a.guess[q.g]);
            Proc P = top_proc(q.d, (int)q.t);
            if (proc_next(P, m, bound)) walk_process(P, q.d, q.w, m, bound, a.h + (size_t)q.g * m, stk, a.status);
        }
        __syncthreads();
        if (tid == 0) qn = 0;
        __syncthreads();
    };
    // persistent workgroups: the queue has to live across buckets
    // each workgroup owns a contiguous range of buckets: the genome (and with it bound and
    // registers) changes rarely and is tracked incrementally -- a binary search plus four dependent
    // scalar loads per bucket cost 16 us of exposed latency per bucket
    const uint32_t per = (a.tb1 - a.tb0 + gridDim.x - 1) / gridDim.x;    // this launch walks buckets [tb0, tb1)
    const uint32_t tb_lo = a.tb0 + blockIdx.x * per, tb_hi = tb_lo + per < a.tb1 ? tb_lo + per : a.tb1;
    if (tb_lo >= tb_hi) return;
    QEntry *gq = LIGHT ? a.gq + a.gq_off[blockIdx.x] : nullptr;
    const uint32_t gq_cap = LIGHT ? (uint32_t)(a.gq_off[blockIdx.x + 1] - a.gq_off[blockIdx.x]) : 0u;
    // the count table is cleared ONCE; afterwards every walk hands it back clean
    for (int e = tid; e < K3_TAB; e += K3_THREADS) { sh.key[e] = K3Key<C32>::EMPTY; sh.cnt[e] = 0; }
    if (tid == 0) sh.ones = 0;
    // counter.h:123 `pair.second > threshold` on integer counts: c > thr  <=>  c >= floor(thr) + 1
    uint32_t cmin = 1;
    if (a.thr >= 1.0) cmin = a.thr >= 4294967295.0 ? 0xFFFFFFFFu : (uint32_t)a.thr + 1u;
    uint32_t g = genome_of_bucket(a.g_boff, a.n, tb_lo), g_end = a.g_boff[g + 1];
    bool skip_g = a.redo_mode && !a.redo[g];
    double bound = V(a.guess[g]);
    uint32_t sbits = a.g_split ? a.g_split[g] : 0u;
    uint32_t bb = C32 ? a.g_bbits[g] : 0u, g_b0 = a.g_boff[g];
    uint64_t o_next = a.bucket_off[tb_lo];
    // Strip 0 = [0, 1) is relevant for EVERY element (counts are >= 1) and has width 1, so the early-out of proc_next,
    // (1 - uu) > bound * 1 * 1.000000001 with uu = ((r1 >> 11) + 1) 2^-53, is an INTEGER test on r1 >> 11: both sides are
    // multiples of 2^-53, 1 - uu exactly.  u0 = smallest r1 >> 11 that is NOT dropped, minus a margin of 2 (whatever passes
    // here takes the unchanged proc_next, which decides): a k-mer seen once costs one xor, one generator step, one compare.
    auto strip0_floor = [](double bnd) -> uint64_t {
        const double b53 = bnd * 1.0 * 1.000000001 * 0x1p53;
        if (!(b53 < 9007199254740988.0)) return 0;                       // large (or NaN) bound: everything goes to the exact test
        if (!(b53 >= 0.)) return 9007199254740989ull;                      // (a negative bound drops everything there too)
        return 9007199254740991ull - 2ull - (uint64_t)b53;
    };
    uint64_t u0 = strip0_floor(bound);
    // total weight = sum of the counts that pass the threshold: integers, summed per thread over the workgroup's buckets
    // of one genome and added to the genome's counter once (exact in any order; no block reduction per bucket)
    uint64_t twi = 0;
    auto flush_tw = [&](uint32_t gg) {
        if (a.redo_mode) { twi = 0; return; }
        uint64_t v = twi;
        for (int o = 32; o; o >>= 1) v += __shfl_xor(v, o);
        if ((tid & 63) == 0 && v) atomicAdd((unsigned long long *)&a.tw_acc[gg], (unsigned long long)v);
        twi = 0;
    };
    __syncthreads();
    for (uint32_t tb = tb_lo; tb < tb_hi; ++tb) {
        const uint64_t o0 = o_next;
        o_next = a.bucket_off[tb + 1];
        const uint64_t nk = o_next - o0;
        if (tb >= g_end) {
            flush_tw(g);
            while (tb >= g_end) { ++g; g_end = a.g_boff[g + 1]; }
            skip_g = a.redo_mode && !a.redo[g];                              // second passes: only genomes whose guess failed
            bound = V(a.guess[g]);
            u0 = strip0_floor(bound);
            sbits = a.g_split ? a.g_split[g] : 0u;
            bb = C32 ? a.g_bbits[g] : 0u; g_b0 = a.g_boff[g];
        }
        if (nk == 0 || skip_g) continue;
        uint64_t *h = a.h + (size_t)g * m;
        // one range of keys: as many table rounds as its size asks for; each round's elements go through phase 1
        auto process = [&](const KT *kb, uint64_t rn, uint32_t shift) -> bool {
            uint32_t R = 1;
            while ((uint64_t)R * a.round_keys < rn) R <<= 1;
            for (uint32_t r = 0; r < R; ++r) {
                // a single round over at most round_keys (< K3_TAB) keys cannot fill the table
                if (R == 1 && rn < (uint64_t)K3_TAB) insert_round<C32, false>(t, kb, rn, 1, 0, shift, bb);
                else if (!insert_round<C32, true>(t, kb, rn, R, r, shift, bb)) return false;
                // Walk the table slots directly, emptying them on the way.  (r01 squeezed the occupied slots into a dense list
                // first -- worth it when the per-element walk was heavy; the compaction, 3.5 ms per call with its three
                // barriers per round, costs more than the 40 % idle lanes here.)
                auto survivor = [&](const Proc &P, uint64_t d, double w, int tt) {
                    const uint32_t slot = atomicAdd(&qn, 1u);
                    if constexpr (LIGHT) {
                        // the region's capacity is twice the expected count; qn keeps counting so that the end of the kernel sees an overflow
                        if (slot < gq_cap) { QEntry *q = gq + slot; q->d = d; q->w = w; q->t = (uint32_t)tt; q->g = g; }
                    } else {
                        if (slot < (uint32_t)K3_QCAP) { queue[slot].d = d; queue[slot].w = w; queue[slot].t = (uint32_t)tt; queue[slot].g = g; }
                        else walk_process(P, d, w, m, bound, h, stk, a.status);   // queue full: do it now
                    }
                };
                auto element = [&](KT key, uint32_t cc) {
                    // the element's id is the masked key (maskfn, src/enums.h:136-140): on the compact path it is formed
                    // here, once per DISTINCT k-mer, from the stored word and the bucket
                    uint64_t d;
                    if constexpr (C32) d = wang64(k3c_kmer(key, tb - g_b0, bb, a.hb) ^ a.xormask);
                    else d = key;
                    twi += cc;
                    uint64_t rng0 = d ^ (0xA0761D6478BD642Full ^ 0x8EBC6AF09C88C6E3ull);      // top_proc(d, 0).rng
                    if ((wy_next(rng0) >> 11) >= u0) {
                        Proc P = top_proc(d, 0);
                        if (proc_next(P, m, bound)) survivor(P, d, (double)cc, 0);
                    }
                    if (cc > 1) {                                        // the strips above [0, 1)
                        const double w = (double)cc;
                        const int nt = top_count(w);
                        for (int tt = 1; tt < nt; ++tt) {
                            Proc P = top_proc(d, tt);
                            if (proc_next(P, m, bound)) survivor(P, d, w, tt);
                        }
                    }
                };
                for (uint32_t e = tid; e < (uint32_t)K3_TAB; e += K3_THREADS) {
                    const uint32_t cc = sh.cnt[e];
                    if (cc) {
                        const KT key = sh.key[e];
                        sh.key[e] = K3Key<C32>::EMPTY; sh.cnt[e] = 0;
                        if (cc >= cmin) element(key, cc);
                    }
                }
                if (tid == 0) {
                    const uint32_t ones = sh.ones;
                    if (ones) { sh.ones = 0; if (ones >= cmin) element(K3Key<C32>::EMPTY, ones); }
                }
                __syncthreads();
                if constexpr (!LIGHT) { if (qn >= (uint32_t)K3_QDRAIN) drain(); }
            }
            return true;
        };
        bool fine;
        if (sbits == 0) {
            fine = process((C32 ? (const KT *)a.keys32 : (const KT *)a.keys) + o0, nk, 0);
        } else {                                             // big inputs: the bucket's pre-split sub-ranges, one after the other
            fine = true;
            const uint64_t sub0 = a.g_sub[g] + ((uint64_t)(tb - a.g_boff[g]) << sbits);
            uint64_t lo = a.sub_off[sub0];
            for (uint32_t rg = 0; rg < (1u << sbits) && fine; ++rg) {
                const uint64_t hi = a.sub_off[sub0 + rg + 1];
                if (hi > lo) fine = process((C32 ? (const KT *)a.skeys32 : (const KT *)a.skeys) + lo, hi - lo, sbits);
                lo = hi;
            }
        }
        if (!fine) { if (tid == 0) atomicExch(a.status, K3_TABLE_OVERFLOW); return; }
        // The bound is never tightened per workgroup: thousands of same-address atomics per genome serialise in L2
        // (measured 25 ms per 4e5 workgroups) and the guess is already within ~2x of the final maximum.
    }
    flush_tw(g);
    __syncthreads();
    if constexpr (LIGHT) {
        if (tid == 0) {
            a.gq_n[blockIdx.x] = qn < gq_cap ? qn : gq_cap;
            if (qn > gq_cap) atomicExch(a.status, K3_REGION_OVERFLOW);                    // the host repeats the pass with the heavy kernel
        }
    } else drain();
}

// the survivors of the light first pass, region by region, one per lane
__global__ __launch_bounds__(K3_THREADS) void k3_bmh_survivor_kernel(BmhArgs a) {
    Proc stk[BMH_STACK];
    const uint32_t n = a.gq_n[blockIdx.x];
    const QEntry *q0 = a.gq + a.gq_off[blockIdx.x];
    for (uint32_t i = threadIdx.x; i < n; i += K3_THREADS) {
        const QEntry q = q0[i];
        const double bound = V(a.guess[q.g]);
        Proc P = top_proc(q.d, (int)q.t);
        if (proc_next(P, a.m, bound)) walk_process(P, q.d, q.w, a.m, bound, a.h + (size_t)q.g * a.m, stk, a.status);
    }
}

// after a pass: was the bound that pruned points at least the final maximum register?  The first
// pass also sums the genome's total weight, from which a failed guess is recomputed.
__global__ __launch_bounds__(K3_THREADS) void k3_bmh_verify_kernel(BmhArgs a) {
    __shared__ uint64_t red[8];
    const uint32_t g = blockIdx.x + a.g0;
    if (a.redo_mode && !a.redo[g]) return;
    const uint64_t hm = block_hmax(a.h + (size_t)g * a.m, a.m, red);
    if (threadIdx.x == 0) {
        double tw;
        if (!a.redo_mode) a.tw[g] = tw = (double)a.tw_acc[g]; else tw = a.tw[g];   // counts: exact below 2^53
        const double guess = V(a.guess[g]);
        const bool bad = tw > 0. && !(V(hm) <= guess);               // no element at all: registers stay +inf, nothing to redo
        a.redo[g] = bad;
        if (bad) {
            const double better = bmh_guess(tw, (double)a.m, (double)__logf((float)a.m));
            a.guess[g] = dbits(better > 16. * guess ? better : 16. * guess);
            atomicAdd(a.nredo, 1u);
        }
    }
}

// R11 alone: distinct (key, count) of every bucket, compacted to the front of the bucket's region
template <bool C32>
__global__ __launch_bounds__(K3_THREADS) void k3_count_kernel(BmhArgs a) {
    typedef typename K3Key<C32>::T KT;
    __shared__ SharedK3<C32> sh;
    const int tid = threadIdx.x;
    const uint32_t tb = blockIdx.x;
    const uint64_t o0 = a.bucket_off[tb], nk = a.bucket_off[tb + 1] - o0;
    if (tid == 0) sh.misc = 0;
    if (nk == 0) { if (tid == 0) a.bucket_nd[tb] = 0; return; }
    const CountTab<C32> t{sh.key, sh.cnt, &sh.ones};
    const uint32_t g = (a.g_split || C32) ? genome_of_bucket(a.g_boff, a.n, tb) : 0u;
    const uint32_t sbits = a.g_split ? a.g_split[g] : 0u;
    const uint32_t bb = C32 ? a.g_bbits[g] : 0u;
    const uint32_t nranges = 1u << sbits;
    const uint64_t sub0 = sbits ? a.g_sub[g] + ((uint64_t)(tb - a.g_boff[g]) << sbits) : 0;
    for (uint32_t rg = 0; rg < nranges; ++rg) {
        const uint64_t lo = sbits ? a.sub_off[sub0 + rg] : o0;
        const uint64_t rn = sbits ? a.sub_off[sub0 + rg + 1] - lo : nk;
        if (rn == 0) continue;
        const KT *kb = (C32 ? (const KT *)(sbits ? a.skeys32 : a.keys32) : (const KT *)(sbits ? a.skeys : a.keys)) + lo;
        uint32_t R = 1;
        while ((uint64_t)R * a.round_keys < rn) R <<= 1;
        for (uint32_t r = 0; r < R; ++r) {
            if (!count_round<C32>(t, kb, rn, R, r, sbits, bb)) { if (tid == 0) atomicExch(a.status, K3_TABLE_OVERFLOW); return; }
            const uint32_t ne = compact_elements<C32>(t, &sh.nelem, a.thr);
            const uint32_t j0 = sh.misc;
            if (a.out_keys)
                for (uint32_t e = tid; e < ne; e += K3_THREADS) {
                    uint64_t key;
                    if constexpr (C32) key = wang64(k3c_kmer(sh.key[e], tb - a.g_boff[g], bb, a.hb) ^ a.xormask);
                    else key = sh.key[e];
                    a.out_keys[o0 + j0 + e] = key; a.out_counts[o0 + j0 + e] = sh.cnt[e];
                }
            __syncthreads();
            if (tid == 0) sh.misc = j0 + ne;
            __syncthreads();
        }
    }
    if (tid == 0) a.bucket_nd[tb] = sh.misc;
}

// K3o (sketch -m c, set space): One-Permutation registers over the k-mers that occur at least c times.  LazyOnePermSetSketch::update
// under set_mincount(c) (reference src/oph.h:154-159,188-205) ends, whatever the order of the k-mers, with register r = the smallest OPH
// id among the DISTINCT k-mers that map to r and occur >= c times (~0 if none): an id is counted for as long as the register is above
// it, and can never win once the register is at or below it.  So the bucket walk of k3_count_kernel selects (the host passes
// thr = c - 1: for integer counts `count > c - 1` is `count >= c`), and every survivor lowers its register with
// global_atomic_umin_x2 behind a plain read, as k3_bmh_main_kernel does.  No LDS stage in front of the atomics: a genome's buckets
// are walked by as many workgroups, each sees ~1/B of the survivors, and of D survivors only ~m ln(D / m) pass the read filter at all.
struct OphMinArgs {
    BmhArgs b;                   // h = the registers [n][m], pre-set to ~0; thr = c - 1; m = d2g_oph_m(S)
    uint64_t ophxor;             // d2g_oph_xor_const()
};

template <bool C32>
__global__ __launch_bounds__(K3_THREADS) void k3_ophmin_kernel(OphMinArgs oa) {
    typedef typename K3Key<C32>::T KT;
    __shared__ SharedK3<C32> sh;
    const BmhArgs &a = oa.b;
    const int tid = threadIdx.x;
    const uint32_t tb = blockIdx.x;
    const uint64_t o0 = a.bucket_off[tb], nk = a.bucket_off[tb + 1] - o0;
    if (nk == 0) return;
    const CountTab<C32> t{sh.key, sh.cnt, &sh.ones};
    const uint32_t g = genome_of_bucket(a.g_boff, a.n, tb);
    const uint32_t sbits = a.g_split ? a.g_split[g] : 0u;
    const uint32_t bb = C32 ? a.g_bbits[g] : 0u;
    const uint32_t nranges = 1u << sbits;
    const uint64_t sub0 = sbits ? a.g_sub[g] + ((uint64_t)(tb - a.g_boff[g]) << sbits) : 0;
    const uint32_t m = a.m;
    const bool pow2 = (m & (m - 1)) == 0;
    const uint64_t ophxor = oa.ophxor;
    uint64_t *hg = a.h + (size_t)g * m;
    for (uint32_t rg = 0; rg < nranges; ++rg) {
        const uint64_t lo = sbits ? a.sub_off[sub0 + rg] : o0;
        const uint64_t rn = sbits ? a.sub_off[sub0 + rg + 1] - lo : nk;
        if (rn == 0) continue;
        const KT *kb = (C32 ? (const KT *)(sbits ? a.skeys32 : a.keys32) : (const KT *)(sbits ? a.skeys : a.keys)) + lo;
        uint32_t R = 1;
        while ((uint64_t)R * a.round_keys < rn) R <<= 1;
        for (uint32_t r = 0; r < R; ++r) {
            if (!count_round<C32>(t, kb, rn, R, r, sbits, bb)) { if (tid == 0) atomicExch(a.status, K3_TABLE_OVERFLOW); return; }
            const uint32_t ne = compact_elements<C32>(t, &sh.nelem, a.thr);
            for (uint32_t e = tid; e < ne; e += K3_THREADS) {
                uint64_t key;
                if constexpr (C32) key = wang64(k3c_kmer(sh.key[e], tb - a.g_boff[g], bb, a.hb) ^ a.xormask);
                else key = sh.key[e];
                const uint64_t id = wang64(key ^ ophxor);                 // DHasher: oph.h:44-53
                const uint32_t idx = pow2 ? ((uint32_t)id & (m - 1)) : ((uint32_t)id % m);   // oph.h:184, as K1
                if (id < hg[idx]) atomicMin((unsigned long long *)&hg[idx], (unsigned long long)id);
            }
            __syncthreads();                                              // the next round clears the table
        }
    }
}

}  // namespace

void k3_init_registers(hipStream_t s, uint64_t *h, size_t nh, double *tw, uint32_t *redo, size_t n) {
    hipLaunchKernelGGL(k3_bmh_init_kernel, dim3((unsigned)div_up<size_t>(std::max(nh, n), K3_THREADS)), dim3(K3_THREADS), 0, s, h, nh, tw, redo, n);
}

namespace {

// the stages behind the buckets of one run (K3Run::run): the run's fields under their own names, and the kernel arguments one stage
// prepares for the next
struct K3Stages {
    K3Run &r;
    d2g_ctx *const ctx = r.ctx; d2g_k3_state *const st = r.st; const hipStream_t s = r.s;
    const K3Host &kh = r.kh; const size_t n = r.n, m = r.m;
    BmhArgs b{};                       // split, count, sketch
    int split(), count(K3Mode mode), ophmin();
    int sketch(const std::vector<size_t> &sub), sketch_init(const std::vector<double> &guess), light_pass(const struct K3LightPlan &plan, bool pipeline);
    void init_registers() { k3_init_registers(s, st->sketch.d_h, n * m, st->sketch.d_tw, st->sketch.d_redo, n); }
};

// big inputs: the buckets of the genomes with gsplit[g] > 0 once more, into table-sized sub-ranges
int K3Stages::split() {
    if (!kh.any_split) return D2G_OK;
    if (int rc = st->count.d_skeys.grow(ctx, std::max<uint64_t>(r.key_words, 1), 4096)) return rc;
    if (int rc = st->count.d_sub_off.grow(ctx, kh.gsub[n] + 1, 4096)) return rc;
    if (int rc = st->count.d_gsplit.grow(ctx, n, 4096)) return rc;
    if (int rc = st->count.d_gsub.grow(ctx, n + 1, 4096)) return rc;
    D2G_HIP(ctx, hipMemcpyAsync(st->count.d_gsplit, kh.gsplit.data(), n * sizeof(uint32_t), hipMemcpyHostToDevice, s));
    D2G_HIP(ctx, hipMemcpyAsync(st->count.d_gsub, kh.gsub.data(), (n + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, s));
    b.g_split = st->count.d_gsplit; b.g_sub = st->count.d_gsub; b.sub_off = st->count.d_sub_off; b.skeys = st->count.d_skeys;
    b.skeys32 = reinterpret_cast<uint32_t *>(st->count.d_skeys.get());
    const unsigned gs = (unsigned)std::min<size_t>(kh.TB, (size_t)ctx->num_cus * 8);
    hipLaunchKernelGGL(kh.compact ? k3_split_kernel<true> : k3_split_kernel<false>, dim3(gs), dim3(K3_THREADS), 0, s, b);
    return D2G_OK;
}

// R11 alone: the distinct (key, count) of every bucket -- K3Mode::Distinct: only how many -- stay in st->count.d_out_* / d_bucket_nd
int K3Stages::count(K3Mode mode) {
    if (mode == K3Mode::Count) {
        if (int rc = st->count.d_out_keys.grow(ctx, std::max<uint64_t>(kh.total, 1), 4096)) return rc;
        if (int rc = st->count.d_out_counts.grow(ctx, std::max<uint64_t>(kh.total, 1), 4096)) return rc;
        b.out_keys = st->count.d_out_keys; b.out_counts = st->count.d_out_counts;
    }
    if (int rc = st->count.d_bucket_nd.grow(ctx, (size_t)kh.TB + 1, 4096)) return rc;
    b.bucket_nd = st->count.d_bucket_nd;
    if (kh.TB) hipLaunchKernelGGL(kh.compact ? k3_count_kernel<true> : k3_count_kernel<false>, dim3(kh.TB), dim3(K3_THREADS), 0, s, b);
    return D2G_OK;
}

// K3o: one workgroup per bucket, as count(); the registers are the caller's
int K3Stages::ophmin() {
    b.h = r.oph_regs;
    const OphMinArgs oa{b, d2g_oph_xor_const()};
    if (kh.TB) hipLaunchKernelGGL(kh.compact ? k3_ophmin_kernel<true> : k3_ophmin_kernel<false>, dim3(kh.TB), dim3(K3_THREADS), 0, s, oa);
    return D2G_OK;
}

// first guess of every genome's bound: with no count threshold the total weight IS the k-mer count; with one it is an upper
// bound (a too small guess only costs a second pass, which then knows the exact weight).  Tests scale it to force the redo path.
std::vector<double> k3_guesses(const K3Host &kh, size_t m, double scale) {
    std::vector<double> guess(kh.gk.size());
    const double lnm = std::log((double)m);
    for (size_t g = 0; g < guess.size(); ++g) guess[g] = scale * bmh_guess((double)std::max<uint64_t>(kh.gk[g], 1), (double)m, lnm);
    return guess;
}
// strips of genome g expected to survive the first pass: at most gk in all (an element of count c has <= c), about gk * guess survive
double k3_survivors(const K3Host &kh, const std::vector<double> &guess, size_t g) { return (double)kh.gk[g] * std::min(1.0, guess[g]); }

// The light first pass as the host plans it: one launch over everything, or one per range of the pipeline.  Survivors go to per-workgroup
// regions of a queue in HBM: gq_scale (twice) the survivors its buckets are expected to produce (a genome's spread evenly over its buckets) + gq_slack
struct LightLaunch { uint32_t t0, t1, g0, g1; unsigned grid; size_t off_at, n_at; uint64_t entry0; };
struct K3LightPlan {
    std::vector<LightLaunch> ll;
    std::vector<uint64_t> off;      // per launch [grid + 1] region offsets relative to the launch's first region (at off_at)
    uint64_t entries = 0; size_t n_words = 0;   // all launches: queue entries; u32 survivor counts, which live behind `off` in the same buffer (n_at indexes u32)
};
K3LightPlan k3_plan_light(const K3Host &kh, const d2g_k3_tuning &t, const std::vector<double> &guess, int num_cus, const std::vector<size_t> &sub) {
    K3LightPlan p;
    const size_t n = kh.gk.size(), nr = sub.size() - 1;
    for (size_t j = 0; j < nr; ++j) {
        LightLaunch L;
        L.g0 = (uint32_t)sub[j]; L.g1 = (uint32_t)sub[j + 1];
        L.t0 = kh.gtab[n + sub[j]]; L.t1 = sub[j + 1] < n ? kh.gtab[n + sub[j + 1]] : kh.TB;
        const size_t cap_grid = std::max<size_t>(1, (size_t)num_cus * t.grid_per_cu / (nr > 1 ? 2 : 1));
        L.grid = (unsigned)std::min<size_t>(std::max<uint32_t>(L.t1 - L.t0, 1), cap_grid);
        L.off_at = p.off.size(); L.n_at = p.n_words; L.entry0 = p.entries;
        // workgroup w of the launch walks buckets [lo, hi) of [t0, t1), as k3_bmh_main_kernel cuts them
        const uint32_t per = (L.t1 - L.t0 + L.grid - 1) / L.grid;
        p.off.resize(L.off_at + L.grid + 1, 0);
        uint64_t *off = p.off.data() + L.off_at;
        size_t g = 0;
        for (unsigned w = 0; w < L.grid; ++w) {
            const uint64_t lo = (uint64_t)L.t0 + (uint64_t)w * per, hi = std::min<uint64_t>(lo + per, L.t1);
            double e = 0.;
            while (g < n && kh.gtab[n + g] + (1ull << kh.gtab[g]) <= lo) ++g;
            for (size_t gg = g; lo < hi && gg < n && kh.gtab[n + gg] < hi; ++gg) {
                const uint64_t b0 = kh.gtab[n + gg], B = 1ull << kh.gtab[gg];
                const uint64_t ov = std::min<uint64_t>(hi, b0 + B) - std::max<uint64_t>(lo, b0);
                e += k3_survivors(kh, guess, gg) * (double)ov / (double)B;
            }
            off[w + 1] = off[w] + (uint64_t)(t.gq_scale * e) + t.gq_slack;
        }
        p.entries += off[L.grid]; p.n_words += L.grid;
        p.ll.push_back(L);
    }
    for (auto &L : p.ll) L.n_at += 2 * p.off.size();
    return p;
}

// buffers of the sketch, the guesses on the device, registers to +inf
int K3Stages::sketch_init(const std::vector<double> &guess) {
    const uint32_t TB = kh.TB;
    if (int rc = st->sketch.d_h.grow(ctx, std::max<size_t>(n * m, 1), 4096)) return rc;
    if (int rc = st->sketch.d_tw.grow(ctx, std::max<size_t>(n, 1), 4096)) return rc;
    if (int rc = st->sketch.d_guess.grow(ctx, std::max<size_t>(n, 1), 4096)) return rc;
    if (int rc = st->sketch.d_redo.grow(ctx, std::max<size_t>(n, 1), 4096)) return rc;
    if (int rc = st->sketch.d_tw_bucket.grow(ctx, (size_t)TB + 1, 4096)) return rc;
    D2G_HIP(ctx, hipMemsetAsync(st->sketch.d_tw_bucket, 0, ((size_t)TB + 1) * sizeof(double), s));
    D2G_HIP(ctx, hipMemcpyAsync(st->sketch.d_guess, guess.data(), n * sizeof(double), hipMemcpyHostToDevice, s));
    b.h = st->sketch.d_h; b.tw = st->sketch.d_tw; b.tw_acc = reinterpret_cast<uint64_t *>(st->sketch.d_tw_bucket.get()); b.guess = st->sketch.d_guess; b.redo = st->sketch.d_redo;
    b.nredo = reinterpret_cast<uint32_t *>(st->count.d_status + 1);
    b.tb0 = 0; b.tb1 = TB; b.g0 = 0;
    init_registers();
    return D2G_OK;
}
// the main kernel of a batch's key form: light (survivors go to the queue in HBM) or heavy (they are walked in place)
auto k3_main_kernel(bool compact, bool light) -> void (*)(BmhArgs) {
    if (!compact) return light ? k3_bmh_main_kernel<false, true> : k3_bmh_main_kernel<false, false>;
    return light ? k3_bmh_main_kernel<true, true> : k3_bmh_main_kernel<true, false>;
}
// the first pass in the light form: main, survivor and verify kernel per planned launch -- pipelined: on the second stream, behind its range's bucketing
int K3Stages::light_pass(const K3LightPlan &plan, bool pipeline) {
    if (pipeline && !st->sketch.xs) {
        D2G_HIP(ctx, st->sketch.xs.create(hipStreamNonBlocking));
        for (auto &e : st->sketch.ev_a) D2G_HIP(ctx, e.create(hipEventDisableTiming));
        D2G_HIP(ctx, st->sketch.ev_b.create(hipEventDisableTiming));
    }
    hipStream_t xs = pipeline ? (hipStream_t)st->sketch.xs : s;
    for (size_t j = 0; j < (pipeline ? plan.ll.size() : 1); ++j) {
        const LightLaunch &L = plan.ll[j];
        BmhArgs x = b;
        x.tb0 = L.t0; x.tb1 = L.t1; x.g0 = L.g0; x.redo_mode = 0;
        x.gq = reinterpret_cast<QEntry *>(st->sketch.d_gq.get()) + L.entry0;
        x.gq_off = st->sketch.d_gq_off + L.off_at;
        x.gq_n = reinterpret_cast<uint32_t *>(st->sketch.d_gq_off.get()) + L.n_at;
        if (pipeline) {
            if (int rc = r.bucket(L.g0, L.g1)) return rc;
            D2G_HIP(ctx, hipEventRecord(st->sketch.ev_a[j], s));
            D2G_HIP(ctx, hipStreamWaitEvent(xs, st->sketch.ev_a[j], 0));
        }
        if (!pipeline || L.t1 > L.t0) {
            hipLaunchKernelGGL(k3_main_kernel(kh.compact, true), dim3(L.grid), dim3(K3_THREADS), 0, xs, x);
            hipLaunchKernelGGL(k3_bmh_survivor_kernel, dim3(L.grid), dim3(K3_THREADS), 0, xs, x);
        }
        if (pipeline) hipLaunchKernelGGL(k3_bmh_verify_kernel, dim3(L.g1 - L.g0), dim3(K3_THREADS), 0, xs, x);
        else hipLaunchKernelGGL(k3_bmh_verify_kernel, dim3((unsigned)n), dim3(K3_THREADS), 0, s, b);
    }
    if (pipeline) {
        D2G_HIP(ctx, hipEventRecord(st->sketch.ev_b, xs));
        D2G_HIP(ctx, hipStreamWaitEvent(s, st->sketch.ev_b, 0));
    }
    return D2G_OK;
}

// R12: registers and total weights of the bucketed batch stay in st->sketch.d_h / st->sketch.d_tw.  `sub`: subbatches()
int K3Stages::sketch(const std::vector<size_t> &sub) {
    const d2g_k3_tuning &t = ctx->k3_tune;
    const uint32_t TB = kh.TB;
    const std::vector<double> guess = k3_guesses(kh, m, t.guess_scale);
    if (int rc = sketch_init(guess)) return rc;
    // Workgroups own contiguous bucket ranges; 6 are resident per CU.  A grid of 8 per CU (r01) left a third of the ranges
    // to a second, three-quarters-empty round: 9.0 ms.  With many more, smaller ranges the hardware's dispatch evens the
    // tail out: 8.3 ms at 6 per CU, 7.9 at 12, 7.6 at 24, 7.3 at 48 and 64 (the survivor kernel follows: 1.9 -> 1.7 ms).
    const unsigned main_grid = (unsigned)std::min<size_t>(TB, (size_t)ctx->num_cus * t.grid_per_cu);
    bool light = TB > 0 && t.light;
    if (light) {
        // batches of read-sized inputs: the bound of a tiny input is above 1 and every element survives -- a queue of
        // 24 bytes per k-mer would buy nothing; such batches keep the heavy form
        double etot = 0.;
        for (size_t g = 0; g < n; ++g) etot += k3_survivors(kh, guess, g);
        if (etot > 0.125 * (double)kh.total) light = false;
    }
    bool pipeline = sub.size() > 2;
    if (pipeline && !light) { if (int rc = r.bucket(0, n)) return rc; pipeline = false; }   // heavy first pass: one range
    K3LightPlan plan;
    if (light) {
        plan = k3_plan_light(kh, t, guess, ctx->num_cus, sub);
        if (int rc = st->sketch.d_gq.grow(ctx, (size_t)plan.entries * (sizeof(QEntry) / 8) + 8, 4096)) return rc;
        if (int rc = st->sketch.d_gq_off.grow(ctx, plan.off.size() + (plan.n_words + 1) / 2 + 1, 4096)) return rc;
        D2G_HIP(ctx, hipMemcpyAsync(st->sketch.d_gq_off, plan.off.data(), plan.off.size() * sizeof(uint64_t), hipMemcpyHostToDevice, s));
    }
    // The first pass walks every genome, light or heavy; a light pass in which a survivor region overflowed (the plan is an expectation) is
    // done AGAIN in the heavy form; redo passes (heavy) then walk the genomes whose guess proved too small, under a larger one, until none is left.
    enum { FirstLight, FirstHeavy, Redo } pass = light ? FirstLight : FirstHeavy;
    for (int redos = 0;;) {
        b.redo_mode = pass == Redo;
        if (pass == FirstLight) { if (int rc = light_pass(plan, pipeline)) return rc; }
        else {
            if (TB) hipLaunchKernelGGL(k3_main_kernel(kh.compact, false), dim3(main_grid), dim3(K3_THREADS), 0, s, b);
            hipLaunchKernelGGL(k3_bmh_verify_kernel, dim3((unsigned)n), dim3(K3_THREADS), 0, s, b);
        }
        int st2[2] = {0, 0};                                  // [0] kernel status, [1] genomes whose guess failed
        D2G_HIP(ctx, hipMemcpyAsync(st2, st->count.d_status, sizeof(st2), hipMemcpyDeviceToHost, s));
        D2G_HIP(ctx, hipStreamSynchronize(s));
        if (pass == FirstLight && st2[0] == K3_REGION_OVERFLOW) {
            D2G_HIP(ctx, hipMemsetAsync(st->count.d_status, 0, 2 * sizeof(int), s));
            D2G_HIP(ctx, hipMemsetAsync(st->sketch.d_tw_bucket, 0, ((size_t)TB + 1) * sizeof(double), s));
            init_registers();
            pass = FirstHeavy;
            continue;
        }
        if (st2[0] || !st2[1]) break;
        D2G_CHECK(ctx, redos < 40, "internal: BagMinHash bound did not converge");
        ++redos; pass = Redo;
        D2G_HIP(ctx, hipMemsetAsync(st->count.d_status + 1, 0, sizeof(int), s));
    }
    return D2G_OK;
}

}  // namespace

int K3Run::run(K3Mode mode) {
    if (km.ftab) {
        // a filtered k-mer is invisible to everything downstream: count the survivors per genome first (one more walk and a host
        // round trip, paid only by filtered calls) and lay the chain out for them
        if (int rc = d2g_filter_survivors(ctx, km, nblk, n, kh.gk.data(), s)) return rc;
        if (int rc = k3_layout_buckets(ctx, n, kh)) return rc;
    }
    if (int rc = upload_tables()) return rc;
    d2g_timer tm(ctx, &ctx->ev_k3, s);
    const std::vector<size_t> sub = subbatches(mode);
    if (int rc = bucket_prepare()) return rc;
    if (sub.size() == 2) if (int rc = bucket(0, n)) return rc;      // pipelined: sketch() buckets range by range
    K3Stages c{*this};
    BmhArgs &b = c.b;
    b.keys = st->count.d_keys; b.keys32 = reinterpret_cast<const uint32_t *>(st->count.d_keys.get()); b.g_bbits = st->count.d_gtab; b.hb = kh.hb; b.xormask = xormask;
    b.bucket_off = st->count.d_bucket_off; b.g_boff = st->count.d_gtab + n;
    b.n = (uint32_t)n; b.TB = kh.TB; b.m = (uint32_t)m; b.thr = thr; b.status = st->count.d_status; b.round_keys = ctx->k3_tune.round_keys;
    if (int rc = c.split()) return rc;
    if (int rc = mode == K3Mode::Sketch ? c.sketch(sub) : mode == K3Mode::OphMin ? c.ophmin() : c.count(mode)) return rc;
    tm.stop();
    D2G_HIP(ctx, hipGetLastError());
    return D2G_OK;
}

// a final status word as the library's error: code and message (K3_REGION_OVERFLOW never leaves sketch())
int k3_status_error(d2g_ctx *ctx, int status) {
    if (status == K3_TABLE_OVERFLOW) { ctx->last_error = "internal: k-mer count table overflow"; return D2G_ERR_INTERNAL; }
    if (status == K3_BAD_WEIGHT) { ctx->last_error = "BagMinHash weight outside (0, 2^53]"; return D2G_ERR_INVALID; }
    if (status == K3_STACK_OVERFLOW) { ctx->last_error = "internal: BagMinHash process stack overflow"; return D2G_ERR_INTERNAL; }
    if (status == K3_SORT_OVERFLOW) { ctx->last_error = "internal: a sort range of the exact k-mer sets outgrew its LDS stage"; return D2G_ERR_INTERNAL; }
    return D2G_OK;
}
int k3_check_status(d2g_ctx *ctx, d2g_k3_state *st, hipStream_t s) {
    int status = 0;
    D2G_HIP(ctx, hipMemcpyAsync(&status, st->count.d_status, sizeof(int), hipMemcpyDeviceToHost, s));
    D2G_HIP(ctx, hipStreamSynchronize(s));
    return k3_status_error(ctx, status);
}

// BagMinHash.  The checks stand in front of the batch (a stage uploads; a refusal comes before it); the operation leaves registers
// [n][sketchsize] and total weights [n] in the state and copies them out as `out` says: device to host or device to device
int bmh_check(d2g_ctx *ctx, size_t n, size_t sketchsize, double count_threshold, const double *sig_out, const double *total_weight_out) {
    D2G_CHECK(ctx, sketchsize >= 1 && sketchsize < (1ull << 24), "sketchsize out of range");
    D2G_CHECK(ctx, (sig_out && total_weight_out) || n == 0, "null output");
    D2G_CHECK(ctx, count_threshold == count_threshold, "count_threshold is NaN");
    return D2G_OK;
}
namespace {
int bmh_sketch(const KmerBatch &b, uint64_t xormask, size_t sketchsize, double count_threshold, double *sig_out, double *total_weight_out,
               hipMemcpyKind out) {
    d2g_ctx *ctx = b.ctx;
    K3Run r;
    if (int rc = k3_begin(b, r)) return rc;
    const size_t n = r.n;
    if (n == 0) return D2G_OK;
    r.xormask = xormask; r.m = sketchsize; r.thr = count_threshold;
    if (int rc = r.run(K3Mode::Sketch)) return rc;
    D2G_HIP(ctx, hipMemcpyAsync(sig_out, r.st->sketch.d_h, n * sketchsize * sizeof(double), out, r.s));
    D2G_HIP(ctx, hipMemcpyAsync(total_weight_out, r.st->sketch.d_tw, n * sizeof(double), out, r.s));
    return k3_check_status(ctx, r.st, r.s);
}
int sketcher_run_bmh(d2g_sketcher *sk, const PackedRuns &in, uint64_t xormask, size_t sketchsize, double count_threshold, double *sig_out,
                     double *total_weight_out) {
    if (!sk) return D2G_ERR_INVALID;
    if (int rc = bmh_check(sk->ctx, in.n, sketchsize, count_threshold, sig_out, total_weight_out)) return rc;
    KmerBatch b;
    if (int rc = d2g_sketcher_stage(sk, in, &b, nullptr)) return rc;
    return bmh_sketch(b, xormask, sketchsize, count_threshold, sig_out, total_weight_out, hipMemcpyDeviceToHost);
}

int sketcher_run_distinct(d2g_sketcher *sk, const PackedRuns &in, uint64_t xormask, uint64_t *ndistinct_out) {
    if (!sk) return D2G_ERR_INVALID;
    d2g_ctx *ctx = sk->ctx;
    const size_t n = in.n;
    D2G_CHECK(ctx, ndistinct_out != nullptr || n == 0, "null output");
    KmerBatch b;
    if (int rc = d2g_sketcher_stage(sk, in, &b, nullptr)) return rc;
    K3Run r;
    if (int rc = k3_begin(b, r)) return rc;
    if (n == 0) return D2G_OK;
    const K3Host &kh = r.kh;
    r.xormask = xormask;
    if (int rc = r.run(K3Mode::Distinct)) return rc;
    if (int rc = k3_check_status(ctx, r.st, r.s)) return rc;
    std::vector<uint32_t> nd(kh.TB);
    D2G_HIP(ctx, hipMemcpyAsync(nd.data(), r.st->count.d_bucket_nd, kh.TB * sizeof(uint32_t), hipMemcpyDeviceToHost, r.s));
    D2G_HIP(ctx, hipStreamSynchronize(r.s));
    for (size_t g = 0; g < n; ++g) {
        uint64_t t = 0;
        for (uint32_t tb = kh.gtab[n + g]; tb < kh.gtab[n + g + 1]; ++tb) t += nd[tb];
        ndistinct_out[g] = t;
    }
    return D2G_OK;
}

}  // namespace

// the exact (key, count) of every bucket of a begun run (n > 0), left in the state: what the count and both set forms read
int k3_exact_counts(K3Run &r, uint64_t xormask, double count_threshold) {
    r.xormask = xormask; r.thr = count_threshold;
    if (int rc = r.run(K3Mode::Count)) return rc;
    return k3_check_status(r.ctx, r.st, r.s);
}

namespace {
// the distinct (key, count) of every genome, compacted on the host (utility form, not the sketch path)
int sketcher_kmer_count(d2g_sketcher *sk, const PackedRuns &in, uint64_t xormask, double count_threshold, uint64_t *keys_out,
                        uint32_t *counts_out, size_t cap, uint64_t *genome_off_out) {
    d2g_ctx *ctx = sk->ctx;
    const size_t n = in.n;
    KmerBatch b;
    if (int rc = d2g_sketcher_stage(sk, in, &b, nullptr)) return rc;
    K3Run r;
    if (int rc = k3_begin(b, r)) return rc;
    const K3Host &kh = r.kh; d2g_k3_state *st = r.st;
    for (size_t g = 0; g <= n; ++g) genome_off_out[g] = 0;
    if (n == 0) return D2G_OK;
    if (int rc = k3_exact_counts(r, xormask, count_threshold)) return rc;
    std::vector<uint32_t> nd(kh.TB);
    std::vector<uint64_t> boff((size_t)kh.TB + 1);
    std::vector<uint64_t> hk(std::max<uint64_t>(kh.total, 1));
    std::vector<uint32_t> hc(std::max<uint64_t>(kh.total, 1));
    D2G_HIP(ctx, hipMemcpy(nd.data(), st->count.d_bucket_nd, kh.TB * sizeof(uint32_t), hipMemcpyDeviceToHost));
    D2G_HIP(ctx, hipMemcpy(boff.data(), st->count.d_bucket_off, ((size_t)kh.TB + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost));
    if (kh.total) {
        D2G_HIP(ctx, hipMemcpy(hk.data(), st->count.d_out_keys, kh.total * sizeof(uint64_t), hipMemcpyDeviceToHost));
        D2G_HIP(ctx, hipMemcpy(hc.data(), st->count.d_out_counts, kh.total * sizeof(uint32_t), hipMemcpyDeviceToHost));
    }
    size_t w = 0;
    for (size_t g = 0; g < n; ++g) {
        genome_off_out[g] = w;
        for (uint32_t tb = kh.gtab[n + g]; tb < kh.gtab[n + g + 1]; ++tb) {
            D2G_CHECK(ctx, w + nd[tb] <= cap, "d2g_kmer_count: output capacity too small");
            std::memcpy(keys_out + w, hk.data() + boff[tb], nd[tb] * sizeof(uint64_t));
            std::memcpy(counts_out + w, hc.data() + boff[tb], nd[tb] * sizeof(uint32_t));
            w += nd[tb];
        }
    }
    genome_off_out[n] = w;
    return D2G_OK;
}

}  // namespace

// K3o behind the entry points of d2g_k1.hip: `regs_dev` [n][m] is pre-set to ~0 on the batch's stream; lowers the registers over the
// k-mers seen at least `mincount` (>= 2) times and waits for the status word
int d2g_k3_ophmin(const KmerBatch &b, uint64_t xormask, size_t m, uint32_t mincount, uint64_t *regs_dev) {
    K3Run r;
    if (int rc = k3_begin(b, r)) return rc;
    if (r.n == 0) return D2G_OK;
    r.xormask = xormask; r.m = m; r.thr = (double)(mincount - 1); r.oph_regs = regs_dev;
    if (int rc = r.run(K3Mode::OphMin)) return rc;
    return k3_check_status(r.ctx, r.st, r.s);
}

extern "C" {

int d2g_sketcher_run_bmh(d2g_sketcher *sk, const uint8_t *packed, size_t packed_bytes, const uint64_t *run_start,
                         const uint32_t *run_len, size_t nrun, const uint64_t *genome_run_off, size_t n, int k, int canon,
                         uint64_t xormask, size_t sketchsize, double count_threshold, double *sig_out,
                         double *total_weight_out) {
    const PackedRuns in{packed, packed_bytes, run_start, run_len, nrun, genome_run_off, n, k, canon};
    return sketcher_run_bmh(sk, in, xormask, sketchsize, count_threshold, sig_out, total_weight_out);
}

int d2g_bmh_sketch_dev(d2g_ctx *ctx, const d2g_oph_plan *plan, const uint8_t *packed_dev, int canon, uint64_t xormask,
                       size_t sketchsize, double count_threshold, double *sig_out_dev, double *total_weight_out_dev,
                       void *stream) {
    if (!ctx || !plan) return D2G_ERR_INVALID;
    if (int rc = bmh_check(ctx, plan->n, sketchsize, count_threshold, sig_out_dev, total_weight_out_dev)) return rc;
    KmerBatch b;
    if (int rc = d2g_plan_batch(ctx, plan, packed_dev, canon, stream, &b)) return rc;
    return bmh_sketch(b, xormask, sketchsize, count_threshold, sig_out_dev, total_weight_out_dev, hipMemcpyDeviceToDevice);
}

int d2g_bmh_sketch(d2g_ctx *ctx, const uint8_t *packed, size_t packed_bytes, const uint64_t *run_start,
                   const uint32_t *run_len, size_t nrun, const uint64_t *genome_run_off, size_t n, int k, int canon,
                   uint64_t xormask, size_t sketchsize, double count_threshold, double *sig_out, double *total_weight_out) {
    const PackedRuns in{packed, packed_bytes, run_start, run_len, nrun, genome_run_off, n, k, canon};
    return d2g_with_sketcher(ctx, [&](d2g_sketcher *sk) {
        return sketcher_run_bmh(sk, in, xormask, sketchsize, count_threshold, sig_out, total_weight_out);
    });
}

int d2g_sketcher_run_distinct(d2g_sketcher *sk, const uint8_t *packed, size_t packed_bytes, const uint64_t *run_start,
                              const uint32_t *run_len, size_t nrun, const uint64_t *genome_run_off, size_t n, int k, int canon,
                              uint64_t xormask, uint64_t *ndistinct_out) {
    const PackedRuns in{packed, packed_bytes, run_start, run_len, nrun, genome_run_off, n, k, canon};
    return sketcher_run_distinct(sk, in, xormask, ndistinct_out);
}

int d2g_kmer_distinct(d2g_ctx *ctx, const uint8_t *packed, size_t packed_bytes, const uint64_t *run_start,
                      const uint32_t *run_len, size_t nrun, const uint64_t *genome_run_off, size_t n, int k, int canon,
                      uint64_t xormask, uint64_t *ndistinct_out) {
    const PackedRuns in{packed, packed_bytes, run_start, run_len, nrun, genome_run_off, n, k, canon};
    return d2g_with_sketcher(ctx, [&](d2g_sketcher *sk) { return sketcher_run_distinct(sk, in, xormask, ndistinct_out); });
}

int d2g_kmer_count(d2g_ctx *ctx, const uint8_t *packed, size_t packed_bytes, const uint64_t *run_start,
                   const uint32_t *run_len, size_t nrun, const uint64_t *genome_run_off, size_t n, int k, int canon,
                   uint64_t xormask, double count_threshold, uint64_t *keys_out, uint32_t *counts_out, size_t cap,
                   uint64_t *genome_off_out) {
    const PackedRuns in{packed, packed_bytes, run_start, run_len, nrun, genome_run_off, n, k, canon};
    if (!ctx) return D2G_ERR_INVALID;
    D2G_CHECK(ctx, genome_off_out != nullptr, "null genome_off_out");
    D2G_CHECK(ctx, cap == 0 || (keys_out && counts_out), "null output");
    return d2g_with_sketcher(ctx, [&](d2g_sketcher *sk) {
        return sketcher_kmer_count(sk, in, xormask, count_threshold, keys_out, counts_out, cap, genome_off_out);
    });
}

}  // extern "C"

void d2g_warm_k3() {
    hipFuncAttributes a;
    (void)hipFuncGetAttributes(&a, reinterpret_cast<const void *>(&k3_bmh_verify_kernel));   // this unit's code object, then the other units'
    d2g_warm_k3_bucket(); d2g_warm_k3_lists(); d2g_warm_k3_sets(); d2g_warm_k3_countsketch();
    d2g_warm_filter();                                                                   // a filtered K3 call counts its survivors first
}
