// d2g_k3_bmh.hip -- K3: the --multiset sketch path on gfx950.
//
//   R11  exact k-mer counting      reference src/counter.h:68-77 (Counter::add(uint64_t)), finalize 118-138,
//                                  driver src/fastxsketch.cpp:425-445
//   R12  BagMinHash                sketch::BagMinHash2<double> (ABSENT dnbaker/sketch bmh.h; parity unpinned);
//                                  restated from Ertl, KDD 2018 under the "BMH-D2G" spec of DESIGN.md
//
// The reference counts with one robin-hood hash map per thread and feeds (kmer, count) to the
// sketch one at a time.  Here:
//   1. k3_hist / k3_scan / k3_scatter / k3_refine : every masked k-mer key = Wang(kmer ^ XORMASK) of a genome is
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
#include "d2g_k1.h"
#include "d2g_countsketch.h"
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <vector>

namespace {

constexpr int K3_THREADS = 256;
constexpr int K3_MAXB = 1 << K3_MAXBBITS;   // buckets per genome (LDS histogram)
constexpr int K3_TAB = 2048;                // LDS count-table slots (24.6 KB with the counts: 6 workgroups per CU)
constexpr uint64_t BMH_INF = 0x7FF0000000000000ull;
constexpr int BMH_STACK = 72;

enum K3Status : int {         // the device status word (d_status[0]): 0 until a kernel raises it
    K3_TABLE_OVERFLOW = 1,    // a round's keys did not fit the LDS count table
    K3_BAD_WEIGHT = 2,        // a weight outside (0, 2^53] (explicit weighted sets)
    K3_STACK_OVERFLOW = 3,    // the BagMinHash descent ran out of its private stack
    K3_REGION_OVERFLOW = 4,   // a survivor region of the light first pass filled up: the host repeats the pass in the heavy form
    K3_SORT_OVERFLOW = 5,     // K3s: a sort range holds more keys than its LDS stage (keys that share their top bits: not hashes)
};

struct K3Args {
    KmerArgs km;
    uint64_t xormask;
    const uint32_t *g_bbits;   // [n]   log2(#buckets) of genome g
    const uint32_t *g_boff;    // [n+1] first global bucket of genome g
    const uint64_t *g_koff;    // [n+1] first key of genome g in `keys` (host prefix of the k-mer counts)
    uint32_t *bucket_cnt;      // [TB]
    uint64_t *bucket_off;      // [TB+1] exclusive prefix of bucket_cnt
    uint64_t *cursor;          // [TB]   scatter cursors (copy of bucket_off)
    uint64_t *keys;            // [total k-mers] bucketed keys
    uint32_t TB;
    // two-level split (genomes with more than 2^l1bits buckets): the scatter writes by the top l1bits of the bucket index
    // only, into `coarse`; k3_refine_kernel then spreads every coarse bucket over its 2^(bb - l1bits) buckets in `keys`
    uint32_t l1bits;
    uint64_t *coarse;          // [total k-mers] or nullptr (no genome needs the second level)
    const uint32_t *l2_tb0;    // [nl2] first bucket of coarse bucket i (global bucket index)
    const uint32_t *l2_bits;   // [nl2] (bb << 8) | (bb - l1bits) of its genome
    uint32_t *blk_coarse;      // [nblk << l1bits] k-mers of launch-plan block b in each of its genome's coarse buckets
    uint32_t g0, n_genomes;    // k3_scan_kernel: first genome of this launch, genomes of the whole batch
};

__device__ __forceinline__ uint32_t bucket_of(uint64_t key, uint32_t bb) { return bb ? (uint32_t)(key >> (64 - bb)) : 0u; }

template <bool FILT, bool WIN = false, bool AA = false>
__global__ __launch_bounds__(K1_THREADS) void k3_hist_kernel(K3Args a) {
    __shared__ uint32_t hist[K3_MAXB];
    const int tid = threadIdx.x;
    const uint32_t blk = blockIdx.x + a.km.blk0;
    const uint32_t g = a.km.blk_genome[blk];
    const uint32_t bb = a.g_bbits[g], B = 1u << bb, boff = a.g_boff[g];
    for (uint32_t i = tid; i < B; i += K1_THREADS) hist[i] = 0;
    __syncthreads();
    const uint64_t xormask = a.xormask;
    d2g_for_each_kmer<FILT, false, WIN, AA>(a.km, [&](uint64_t x) {
        const uint64_t key = wang64(x ^ xormask);              // maskfn: src/enums.h:136-140
        atomicAdd(&hist[bucket_of(key, bb)], 1u);
    });
    __syncthreads();
    for (uint32_t i = tid; i < B; i += K1_THREADS)
        if (hist[i]) atomicAdd(&a.bucket_cnt[boff + i], hist[i]);
    // the workgroup's count per COARSE bucket (the scatter's write fronts): saves the scatter its counting enumeration
    const uint32_t b1 = bb < a.l1bits ? bb : a.l1bits, sb = bb - b1;
    uint32_t *mine = a.blk_coarse + ((size_t)blk << a.l1bits);
    for (uint32_t i = tid; i < (1u << b1); i += K1_THREADS) {
        uint32_t c = 0;
        for (uint32_t j = 0; j < (1u << sb); ++j) c += hist[(i << sb) + j];
        mine[i] = c;
    }
}

// exclusive prefix of bucket_cnt: one workgroup per genome scans its <= 4096 buckets (coalesced, 16 per
// lane); the genome's first key offset comes from the host, which knows every genome's k-mer count
__global__ __launch_bounds__(K3_THREADS) void k3_scan_kernel(K3Args a) {
    __shared__ uint32_t wsum[K3_THREADS / 64];
    const uint32_t tid = threadIdx.x, g = blockIdx.x + a.g0;
    const uint32_t b0 = a.g_boff[g], B = a.g_boff[g + 1] - b0;
    const uint32_t per = (B + K3_THREADS - 1) / K3_THREADS;             // <= 16
    const uint32_t lo = min(B, tid * per), hi = min(B, lo + per);
    uint32_t s = 0;
    for (uint32_t i = lo; i < hi; ++i) s += a.bucket_cnt[b0 + i];
    uint32_t incl = s;                                                  // inclusive scan across the wave, then the 4 waves
    for (int o = 1; o < 64; o <<= 1) { const uint32_t v = __shfl_up(incl, o); if ((tid & 63) >= (uint32_t)o) incl += v; }
    if ((tid & 63) == 63) wsum[tid >> 6] = incl;
    __syncthreads();
    uint32_t wbase = 0;
    for (uint32_t w = 0; w < (tid >> 6); ++w) wbase += wsum[w];
    uint64_t run = a.g_koff[g] + wbase + (incl - s);
    for (uint32_t i = lo; i < hi; ++i) {
        a.bucket_off[b0 + i] = run; a.cursor[b0 + i] = run;
        run += a.bucket_cnt[b0 + i];
    }
    // the end of this launch's last bucket = the first key of the next genome (the whole batch: bucket_off[TB]).  A later
    // launch over the next genomes writes the same value there; the counting pass of THIS range may already be reading it.
    if (blockIdx.x == gridDim.x - 1 && tid == K3_THREADS - 1) a.bucket_off[b0 + B] = a.g_koff[g + 1];
}

// Write-combining decides this pass.  A workgroup's 65 536 k-mers leave ~16 keys = one 128-byte line in each of 4096
// buckets, but every 8-byte store is a separate partial write and 4096 open lines per workgroup x 160 workgroups per XCD
// do not live in a 4 MB L2 until they are full: measured 38 GB of HBM writes for 10 GB of keys, 14.4 ms.  With <= 256
// write fronts per workgroup most lines are completed first (6.4 ms at 256 fronts, 5.1 ms at 64; the number of workgroups per
// CU makes no difference, 2 or 8: it is the fronts one workgroup keeps open that count).  So
// genomes with more than 2^l1bits buckets are split in two levels: here by the top l1bits of the bucket index -- the
// coarse bucket's region is the union of its buckets' regions, reserved through the cursor of its first bucket -- and
// then by the remaining bits, per coarse bucket, in k3_refine_kernel (<= 2^(12 - l1bits) fronts per workgroup there).
template <bool FILT, bool WIN = false, bool AA = false>
__global__ __launch_bounds__(K1_THREADS) void k3_scatter_kernel(K3Args a) {
    // ONE LDS array: first the workgroup's count per (coarse) bucket, then (after one 64-bit reservation
    // per bucket) the next write position relative to the genome's first key -- a genome holds < 2^32
    // k-mers -- so that a key's slot is a single LDS atomic.
    __shared__ uint32_t pos[K3_MAXB];
    const int tid = threadIdx.x;
    const uint32_t blk = blockIdx.x + a.km.blk0;
    const uint32_t g = a.km.blk_genome[blk];
    const uint32_t bb = a.g_bbits[g], boff = a.g_boff[g];
    const uint32_t b1 = bb < a.l1bits ? bb : a.l1bits, sb = bb - b1, B = 1u << b1;
    const uint64_t koff = a.g_koff[g];
    const uint64_t xormask = a.xormask;
    const uint32_t *mine = a.blk_coarse + ((size_t)blk << a.l1bits);              // counted by k3_hist_kernel
    for (uint32_t i = tid; i < B; i += K1_THREADS) {
        const uint32_t c = mine[i];
        pos[i] = c ? (uint32_t)(atomicAdd((unsigned long long *)&a.cursor[boff + (i << sb)], (unsigned long long)c) - koff) : 0u;
    }
    __syncthreads();
    uint64_t *keys = (sb ? a.coarse : a.keys) + koff;
    d2g_for_each_kmer<FILT, false, WIN, AA>(a.km, [&](uint64_t x) {
        const uint64_t key = wang64(x ^ xormask);
        const uint32_t slot = atomicAdd(&pos[bucket_of(key, b1)], 1u);
        keys[slot] = key;
    });
}

// second level: one workgroup per coarse bucket; the offsets of its 2^sb buckets are known from the histogram pass, so
// this is ONE read of the region and one LDS atomic per key
__global__ __launch_bounds__(K3_THREADS) void k3_refine_kernel(K3Args a) {
    __shared__ uint32_t pos[K3_MAXB];
    const uint32_t tid = threadIdx.x;
    const uint32_t tb0 = a.l2_tb0[blockIdx.x], bits = a.l2_bits[blockIdx.x];
    const uint32_t bb = bits >> 8, sb = bits & 255u, R = 1u << sb;
    const uint64_t o0 = a.bucket_off[tb0], nk = a.bucket_off[tb0 + R] - o0;
    for (uint32_t i = tid; i < R; i += K3_THREADS) pos[i] = (uint32_t)(a.bucket_off[tb0 + i] - o0);
    __syncthreads();
    const uint64_t *src = a.coarse + o0;
    uint64_t *dst = a.keys + o0;
    constexpr int PF = 8;                    // 4 and 16 measured: no difference (the pass moves 20 GB: bandwidth)
    for (uint64_t b0 = 0; b0 < nk; b0 += (uint64_t)PF * K3_THREADS) {
        uint64_t kk[PF];
#pragma unroll
        for (int j = 0; j < PF; ++j) { const uint64_t i = b0 + (uint64_t)j * K3_THREADS + tid; kk[j] = i < nk ? src[i] : 0; }
#pragma unroll
        for (int j = 0; j < PF; ++j)
            if (b0 + (uint64_t)j * K3_THREADS + tid < nk) dst[atomicAdd(&pos[bucket_of(kk[j], bb) & (R - 1)], 1u)] = kk[j];
    }
}

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

struct K3cArgs {
    KmerArgs km;
    const uint32_t *g_bbits;   // [n]
    const uint32_t *g_boff;    // [n+1] first global bucket of genome g
    const uint64_t *g_koff;    // [n+1] first k-mer slot of genome g
    const uint32_t *g_blk;     // [n+1] first workgroup (launch-plan block) of genome g
    uint16_t *tile_cnt;        // [ntiles][K3C_MAXB] k-mers of tile (block * K1_CPT + it) per bucket
    uint32_t *tile_off;        // [ntiles][K3C_MAXB] write offset of that tile in the bucket, relative to the genome's first slot
    uint32_t *bucket_cnt;      // [TB]
    uint64_t *bucket_off;      // [TB+1]
    uint32_t *keys32;          // [total k-mers]
    uint32_t hb;               // hi bits = max(0, d2g_key_bits(k, alphabet) - 32): 2k - 32 for DNA
    uint32_t TB;
};

template <bool FILT, bool WIN = false, bool AA = false>
__global__ __launch_bounds__(K1_THREADS) void k3c_hist_kernel(K3cArgs a) {
    __shared__ uint32_t cnt[K3C_MAXB];
    const int tid = threadIdx.x;
    const uint32_t g = a.km.blk_genome[blockIdx.x];
    const uint32_t bb = a.g_bbits[g], B = 1u << bb, hb = a.hb;
    for (int it = 0; it < K1_CPT; ++it) {
        for (uint32_t i = tid; i < B; i += K1_THREADS) cnt[i] = 0;
        __syncthreads();
        d2g_for_each_kmer_its<FILT, false, WIN, AA>(a.km, it, it + 1, [&](uint64_t x) { atomicAdd(&cnt[k3c_bucket(x, bb, hb)], 1u); });
        __syncthreads();
        // a tile holds at most 16384 k-mers: the counts fit u16
        uint16_t *dst = a.tile_cnt + ((size_t)blockIdx.x * K1_CPT + it) * K3C_MAXB;
        for (uint32_t i = tid; i < B; i += K1_THREADS) dst[i] = (uint16_t)cnt[i];
        __syncthreads();
    }
}

// one workgroup per genome: bucket totals over the genome's tiles -> exclusive prefix over buckets -> bucket offsets,
// then per tile and bucket the offset at which that tile writes
__global__ __launch_bounds__(K3_THREADS) void k3c_scan_kernel(K3cArgs a) {
    __shared__ uint32_t wsum[K3_THREADS / 64];
    constexpr int PER = K3C_MAXB / K3_THREADS;                       // 4 consecutive buckets per thread
    const uint32_t tid = threadIdx.x, g = blockIdx.x;
    const uint32_t bb = a.g_bbits[g], B = 1u << bb, b0 = a.g_boff[g];
    const size_t t0 = (size_t)a.g_blk[g] * K1_CPT, t1 = (size_t)a.g_blk[g + 1] * K1_CPT;
    uint32_t tot[PER];
#pragma unroll
    for (int j = 0; j < PER; ++j) tot[j] = 0;
    for (size_t t = t0; t < t1; ++t) {
        const uint16_t *c = a.tile_cnt + t * K3C_MAXB + tid * PER;
#pragma unroll
        for (int j = 0; j < PER; ++j) if (tid * PER + j < B) tot[j] += c[j];
    }
    uint32_t s = 0;
#pragma unroll
    for (int j = 0; j < PER; ++j) s += tot[j];
    uint32_t incl = s;
    for (int o = 1; o < 64; o <<= 1) { const uint32_t v = __shfl_up(incl, o); if ((tid & 63) >= (uint32_t)o) incl += v; }
    if ((tid & 63) == 63) wsum[tid >> 6] = incl;
    __syncthreads();
    uint32_t run = incl - s;
    for (uint32_t w = 0; w < (tid >> 6); ++w) run += wsum[w];
    uint32_t base[PER];
#pragma unroll
    for (int j = 0; j < PER; ++j) {
        base[j] = run;
        if (tid * PER + j < B) { a.bucket_off[b0 + tid * PER + j] = a.g_koff[g] + run; a.bucket_cnt[b0 + tid * PER + j] = tot[j]; }
        run += tot[j];
    }
    if (g == gridDim.x - 1 && tid == K3_THREADS - 1) a.bucket_off[a.TB] = a.g_koff[g + 1];
    for (size_t t = t0; t < t1; ++t) {
        const uint16_t *c = a.tile_cnt + t * K3C_MAXB + tid * PER;
        uint32_t *o = a.tile_off + t * K3C_MAXB + tid * PER;
#pragma unroll
        for (int j = 0; j < PER; ++j) if (tid * PER + j < B) { o[j] = base[j]; base[j] += c[j]; }
    }
}

// LDS: the tile's 16384 stored words sorted by bucket, the tile-local first slot of each bucket, and a cursor
struct K3cScatterLds {
    uint32_t stage[K3C_TILE];
    uint32_t lbase[K3C_MAXB + 1];
    uint32_t lcur[K3C_MAXB];
    uint32_t wsum[K1_THREADS / 64];
};

template <bool FILT, bool WIN = false, bool AA = false>
__global__ __launch_bounds__(K1_THREADS) void k3c_scatter_kernel(K3cArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char k3c_lds_raw[];
    K3cScatterLds &L = *reinterpret_cast<K3cScatterLds *>(k3c_lds_raw);
    constexpr int PER = K3C_MAXB / K1_THREADS;
    const uint32_t tid = threadIdx.x;
    const uint32_t g = a.km.blk_genome[blockIdx.x];
    const uint32_t bb = a.g_bbits[g], B = 1u << bb, hb = a.hb;
    uint32_t *out = a.keys32 + a.g_koff[g];
    for (int it = 0; it < K1_CPT; ++it) {
        const size_t tile = (size_t)blockIdx.x * K1_CPT + it;
        // tile-local exclusive prefix of the bucket counts
        const uint16_t *c = a.tile_cnt + tile * K3C_MAXB + tid * PER;
        uint32_t cnt[PER], s = 0;
#pragma unroll
        for (int j = 0; j < PER; ++j) { cnt[j] = (tid * PER + j < B) ? c[j] : 0u; s += cnt[j]; }
        uint32_t incl = s;
        for (int o = 1; o < 64; o <<= 1) { const uint32_t v = __shfl_up(incl, o); if ((tid & 63) >= (uint32_t)o) incl += v; }
        if ((tid & 63) == 63) L.wsum[tid >> 6] = incl;
        __syncthreads();
        uint32_t run = incl - s, total = 0;
        for (uint32_t w = 0; w < K1_THREADS / 64; ++w) { if (w < (tid >> 6)) run += L.wsum[w]; total += L.wsum[w]; }
#pragma unroll
        for (int j = 0; j < PER; ++j) { L.lbase[tid * PER + j] = run; L.lcur[tid * PER + j] = run; run += cnt[j]; }
        if (tid == K1_THREADS - 1) L.lbase[K3C_MAXB] = run;
        __syncthreads();
        if (total == 0) continue;                                    // uniform: every thread computed the same total
        d2g_for_each_kmer_its<FILT, false, WIN, AA>(a.km, it, it + 1, [&](uint64_t x) {
            L.stage[atomicAdd(&L.lcur[k3c_bucket(x, bb, hb)], 1u)] = (uint32_t)x;
        });
        __syncthreads();
        // flush: runs average 16 words, so a quarter wave (16 lanes) copies one bucket's run at a time -- a wave
        // store covers four runs of ~64 B; no per-element search for the bucket
        const uint32_t *toff = a.tile_off + tile * K3C_MAXB;
        const uint32_t q = tid >> 4, l16 = tid & 15;                 // 16 quarter-waves per workgroup
        for (uint32_t b = q; b < B; b += K1_THREADS / 16) {
            const uint32_t r0 = L.lbase[b], r1 = L.lbase[b + 1];
            if (r0 == r1) continue;
            uint32_t *dst = out + toff[b];
            for (uint32_t i = r0 + l16; i < r1; i += 16) dst[i - r0] = L.stage[i];
        }
        __syncthreads();
    }
}

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

// The main pass splits the walk in two.  Phase 1 (every element, every lane): the first point of
// each relevant top strip; 99% die in the early-out of proc_next.  A survivor needs the ~60-level
// descent of bmh_locate, which one lane would run alone while 63 wait -- so survivors are queued in
// LDS and phase 2 drains the queue with one survivor per lane once enough have accumulated.
struct QEntry { uint64_t d; double w; uint32_t t, g; };     // strip t of element (d, w) of genome g: the survivor's
                                                             // process is regenerated in phase 2 (24 B instead of 56)
constexpr int K3_QCAP = 256;
constexpr int K3_QDRAIN = 160;          // drain when at least this many are waiting

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

__device__ __forceinline__ uint32_t genome_of_bucket(const uint32_t *g_boff, uint32_t n, uint32_t tb) {
    uint32_t lo = 0, hi = n;
    while (hi - lo > 1) { const uint32_t mid = (lo + hi) >> 1; if (g_boff[mid] <= tb) lo = mid; else hi = mid; }
    return lo;
}

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

// the pruning bound for total weight W: the final maximum register is the max of m exponentials of
// rate W/m -- mean (m/W)(ln m + 0.58), sd 1.28 m/W; 1.25 x (mean + 6 sd) fails about once in 4000 genomes
__host__ __device__ inline double bmh_guess(double W, double m, double lnm) { return 1.25 * (m / W) * (lnm + 0.58 + 8.0); }

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

// ---------------------------------------------------------------------------------------------
// explicit weighted sets (wsketch.cpp:54-73 minwise_det / 17-51 rowwise CSR): elements come
// from (id, weight) arrays instead of the count table
// ---------------------------------------------------------------------------------------------
struct WsArgs {
    const uint64_t *ids;
    const double *w;             // nullptr => 1.0
    const uint32_t *blk_set;     // set of workgroup
    const uint64_t *blk_lo;      // first element
    const uint32_t *blk_cnt;     // element count
    uint32_t m;
    uint64_t *h;                 // [nsets][m]
    const uint64_t *guess;       // [nsets] pruning bound of this pass
    const uint32_t *redo;        // [nsets] (redo_mode) sets to walk again
    int redo_mode;
    int *status;
    uint64_t *arg;               // argmin pass: [nsets][m] owner positions, pre-set to ~0
    const uint64_t *set_lo;      // argmin pass: [nsets] first element of each set
};

__device__ __forceinline__ bool ws_fetch(const WsArgs &a, uint64_t idx, uint64_t &d, double &w, int *status) {
    d = a.ids[idx];
    w = a.w ? a.w[idx] : 1.0;
    if (!(w > 0.)) return false;                                   // BagMinHash2::update ignores w <= 0
    if (!(w <= 0x1p53)) { atomicExch(status, K3_BAD_WEIGHT); return false; }   // outside the level set (also NaN)
    return true;
}

__global__ __launch_bounds__(K3_THREADS) void k3_bmh_sets_kernel(WsArgs a) {
    const uint32_t set = a.blk_set[blockIdx.x];
    if (a.redo_mode && !a.redo[set]) return;
    const uint64_t lo = a.blk_lo[blockIdx.x], cnt = a.blk_cnt[blockIdx.x];
    const double bound = V(a.guess[set]);
    uint64_t *hg = a.h + (size_t)set * a.m;
    Proc stk[BMH_STACK];
    for (uint64_t e = threadIdx.x; e < cnt; e += K3_THREADS) {
        uint64_t d; double w;
        if (ws_fetch(a, lo + e, d, w, a.status)) walk_element(d, w, a.m, bound, hg, stk, a.status);
    }
}

// after the registers are final: one more walk under the verified bound records, per register, the position
// (within its set) of the element whose point it holds
__global__ __launch_bounds__(K3_THREADS) void k3_bmh_sets_argmin_kernel(WsArgs a) {
    const uint32_t set = a.blk_set[blockIdx.x];
    const uint64_t lo = a.blk_lo[blockIdx.x], cnt = a.blk_cnt[blockIdx.x];
    const double bound = V(a.guess[set]);
    Proc stk[BMH_STACK];
    for (uint64_t e = threadIdx.x; e < cnt; e += K3_THREADS) {
        uint64_t d; double w;
        if (ws_fetch(a, lo + e, d, w, a.status))
            walk_element(d, w, a.m, bound, ArgSink{a.h + (size_t)set * a.m, a.arg + (size_t)set * a.m, lo + e - a.set_lo[set]}, stk, a.status);
    }
}

// per set: max(h) <= guess ?  else raise the guess and flag the set
__global__ __launch_bounds__(K3_THREADS) void k3_sets_verify_kernel(const uint64_t *h, uint32_t m, uint64_t *guess, uint32_t *redo,
                                                                   const double *tw, uint32_t *nredo, int redo_mode) {
    __shared__ uint64_t red[8];
    const uint32_t set = blockIdx.x;
    if (redo_mode && !redo[set]) return;
    const uint64_t hm = block_hmax(h + (size_t)set * m, m, red);
    if (threadIdx.x == 0) {
        const double g = V(guess[set]);
        const bool bad = tw[set] > 0. && !(V(hm) <= g);
        redo[set] = bad;
        if (bad) { guess[set] = dbits(16. * g); atomicAdd(nredo, 1u); }
    }
}

// the first guess of every set's bound from its total weight, as bit patterns (0 for a set without weight: nothing is walked)
std::vector<uint64_t> ws_guesses(const double *tw, size_t nsets, size_t m, double scale) {
    std::vector<uint64_t> guess(nsets);
    const double lnm = std::log((double)m);
    for (size_t i = 0; i < nsets; ++i) {
        const double gv = tw[i] > 0. ? scale * bmh_guess(tw[i], (double)m, lnm) : 0.;
        std::memcpy(&guess[i], &gv, 8);
    }
    return guess;
}
// The passes over explicit sets whose lists, workgroup tables, guesses, total weights and +inf registers are ON THE DEVICE (host
// arrays uploaded by d2g_bmh_from_weighted_ids, or the lists K3k compacted there): every set under its guess, the verification, the
// sets that failed it again under a guess 16 times larger, until none is left.  Synchronises `s` once per pass, for the two words of d_status.
int ws_walk(d2g_ctx *ctx, hipStream_t s, WsArgs &a, size_t nsets, size_t nb, uint64_t *d_guess, uint32_t *d_redo, const double *d_tw, int *d_status) {
    for (int pass = 0;; ++pass) {
        a.redo_mode = pass > 0;
        if (nb) hipLaunchKernelGGL(k3_bmh_sets_kernel, dim3((unsigned)nb), dim3(K3_THREADS), 0, s, a);
        hipLaunchKernelGGL(k3_sets_verify_kernel, dim3((unsigned)nsets), dim3(K3_THREADS), 0, s, a.h, a.m, d_guess, d_redo, d_tw,
                           reinterpret_cast<uint32_t *>(d_status + 1), a.redo_mode);
        int st2[2] = {0, 0};
        D2G_HIP(ctx, hipMemcpyAsync(st2, d_status, sizeof(st2), hipMemcpyDeviceToHost, s));
        D2G_HIP(ctx, hipStreamSynchronize(s));
        if (st2[0] || !st2[1]) break;
        if (pass >= 40) { ctx->last_error = "internal: BagMinHash bound did not converge"; return D2G_ERR_INTERNAL; }
        D2G_HIP(ctx, hipMemsetAsync(d_status + 1, 0, sizeof(int), s));
    }
    return D2G_OK;
}

uint32_t ceil_log2(uint64_t x) { uint32_t b = 0; while ((1ull << b) < x) ++b; return b; }

}  // namespace

// grow-only work buffers of the --multiset path (owned by a sketcher or by a one-shot call)
struct d2g_k3_state {
    d2g_dev<uint32_t> d_gtab;        // g_bbits [n] + g_boff [n+1]
    d2g_dev<uint64_t> d_koff;        // [n+1]
    d2g_dev<uint32_t> d_bucket_cnt;
    d2g_dev<uint64_t> d_bucket_off;
    d2g_dev<uint64_t> d_cursor;
    d2g_dev<uint32_t> d_l2;     // two-level split: coarse bucket table
    d2g_dev<uint32_t> d_blk_coarse;
    d2g_dev<uint64_t> d_gq;     // survivors of the light first pass (QEntry)
    d2g_dev<uint64_t> d_gq_off;   // [grid+1] region offsets, then [grid] u32 counts
    d2g_stream xs;                                   // second stream of the sub-batch pipeline
    d2g_event ev_a[8], ev_b;
    d2g_dev<uint64_t> d_keys;
    d2g_dev<uint64_t> d_skeys;      // big inputs: keys regrouped by sub-range
    d2g_dev<uint32_t> d_gblk;        // compact path: first launch-plan block of each genome
    d2g_dev<uint16_t> d_tile_cnt;
    d2g_dev<uint32_t> d_tile_off;
    d2g_dev<uint64_t> d_sub_off;
    d2g_dev<uint32_t> d_gsplit;
    d2g_dev<uint64_t> d_gsub;
    d2g_dev<uint64_t> d_h;
    d2g_dev<double> d_tw;
    d2g_dev<int> d_status;                 // [0] status, [1] nredo
    d2g_dev<uint64_t> d_guess;
    d2g_dev<double> d_tw_bucket;
    d2g_dev<uint32_t> d_redo;
    d2g_dev<uint32_t> d_out_counts;
    d2g_dev<uint32_t> d_bucket_nd;
    d2g_dev<uint64_t> d_out_keys;
    // K3s, the sorted emission (d2g_kmer_sets*)
    d2g_dev<uint32_t> d_ks_pbits;    // [n] log2(sort ranges) of genome g
    d2g_dev<uint64_t> d_ks_rbase;    // [n+1] first sort range of genome g
    d2g_dev<uint32_t> d_ks_cnt;      // [nranges]
    d2g_dev<uint64_t> d_ks_off;      // [nranges+1]
    d2g_dev<uint64_t> d_ks_cur;      // [nranges]
    d2g_dev<uint64_t> d_ks_setoff;   // [n+1]
    d2g_dev<uint64_t> d_ks_cards;    // [n][2]
    d2g_dev<uint64_t> d_ks_keys;     // host-pointer form: the sorted keys ...
    d2g_dev<uint32_t> d_ks_counts;   // ... and counts (also the count column of a caller that asked for keys only)
    // K3k, the count-sketch (d2g_bmh_sketch_cs*, d2g_countsketch_*)
    d2g_dev<int32_t> d_cs_table;     // [rows of one group][cells], zeroed per group for exactly rows * cells cells
    d2g_dev<uint32_t> d_cs_row;      // [n] the table row of genome g inside its group
    d2g_dev<uint32_t> d_cs_tile_cnt; // [rows * tiles] cells kept per tile of K3K_TILE cells
    d2g_dev<uint64_t> d_cs_tile_off; // [rows * tiles + 1] their exclusive prefix, then row_off [rows + 1], then the total weight [rows]
    d2g_dev<uint64_t> d_cs_ids;      // the lists of one group: cell numbers, each row's ascending ...
    d2g_dev<double> d_cs_w;          // ... and |count|
    d2g_dev<uint64_t> d_cs_blo;      // BagMinHash over them: the workgroup tables (d2g_ws_blocks) ...
    d2g_dev<uint32_t> d_cs_bset;     // ... set [nb], then cnt [nb]
};

void d2g_k3_state_destroy(d2g_k3_state *st) { delete st; }

namespace {

struct K3Host {
    std::vector<uint32_t> gtab;        // bbits[n] then boff[n+1]
    std::vector<uint64_t> gk;          // k-mers per genome
    std::vector<uint64_t> koff;        // [n+1] exclusive prefix of gk
    std::vector<uint32_t> gsplit;      // [n] log2(sub-ranges per bucket) of big genomes, 0 otherwise
    std::vector<uint64_t> gsub;        // [n+1] first sub-range of genome g
    std::vector<uint32_t> gblk;        // [n+1] first launch-plan block of genome g (compact path)
    bool compact = false;              // k <= 21: 4-byte stored words + tile-sorted split (k3c_*)
    uint32_t hb = 0;                   // compact path: hi bits = max(0, d2g_key_bits(k, alphabet) - 32): 2k - 32 for DNA
    bool any_split = false;
    uint64_t total = 0;
    uint32_t TB = 0;
    uint32_t l1bits = K3_L1BITS;        // generic path: bucket bits the scatter resolves itself
    std::vector<uint32_t> l2_tb0, l2_bits;   // coarse buckets that k3_refine_kernel spreads over their buckets
    std::vector<uint32_t> l2_start;          // [n+1] first entry of genome g in the two arrays above
};

int k3_layout_buckets(d2g_ctx *ctx, size_t n, K3Host &kh);
// k-mers and launch-plan blocks per genome from the run table, then the bucket layout those k-mer counts ask for
int k3_layout(d2g_ctx *ctx, const PackedRuns &in, K3Host &kh) {
    const d2g_k3_tuning &t = ctx->k3_tune;
    const size_t n = in.n;
    const int k = in.k;
    kh.gk.assign(n, 0);
    kh.gblk.assign(n + 1, 0);
    const int key_bits = d2g_key_bits(k, in.alphabet);             // DNA: 2k; a protein alphabet: the bit length of A^k - 1
    kh.hb = key_bits > 32 ? (uint32_t)(key_bits - 32) : 0u;
    // the compact path (4-byte stored words, tile-sorted split) halves the chain's HBM traffic but is ~11 % slower end to
    // end (one Wang mix per distinct k-mer moves into the issue-bound main pass): opt-in with D2G_K3_COMPACT=1, k <= 21
    kh.compact = t.compact && kh.hb <= (uint32_t)K3C_MAXBBITS;
    for (size_t g = 0; g < n; ++g) {
        uint64_t nk = 0, chunks = 0;
        for (uint64_t r = in.genome_run_off[g]; r < in.genome_run_off[g + 1]; ++r) {
            const uint64_t rk = d2g_run_emissions_of(in.run_len[r], k, in.w);
            nk += rk; chunks += div_up<uint64_t>(rk, K1_CHUNK);
        }
        D2G_CHECK(ctx, nk < (1ull << 32), "--multiset: more than 2^32 k-mers in one input");
        kh.gk[g] = nk;
        kh.gblk[g + 1] = kh.gblk[g] + (uint32_t)div_up<uint64_t>(chunks, K1_BLOCK_CHUNKS);
    }
    return k3_layout_buckets(ctx, n, kh);
}
// everything that follows from kh.gk: buckets, key offsets, sub-ranges.  Run again by K3Run::run when a k-mer filter is attached,
// over the k-mers that SURVIVE it -- the chain then lays out, guesses and splits exactly as for an input that never held the others.
int k3_layout_buckets(d2g_ctx *ctx, size_t n, K3Host &kh) {
    const d2g_k3_tuning &t = ctx->k3_tune;
    kh.gtab.assign(2 * n + 1, 0);
    kh.total = 0; kh.any_split = false;
    uint64_t tb = 0;
    kh.l1bits = t.l1bits; kh.l2_tb0.clear(); kh.l2_bits.clear(); kh.l2_start.assign(n + 1, 0);
    for (size_t g = 0; g < n; ++g) {
        const uint64_t nk = kh.gk[g];
        kh.total += nk;
        uint32_t bb;
        if (kh.compact) bb = std::max<uint32_t>(kh.hb, std::min<uint32_t>(K3C_MAXBBITS, ceil_log2((nk + K3C_TARGET - 1) / K3C_TARGET)));
        else bb = std::min<uint32_t>(K3_MAXBBITS, ceil_log2((nk + t.bucket_keys - 1) / t.bucket_keys));
        kh.gtab[g] = bb;
        kh.gtab[n + g] = (uint32_t)tb;
        kh.l2_start[g] = (uint32_t)kh.l2_tb0.size();
        if (!kh.compact && bb > kh.l1bits)
            for (uint32_t c = 0; c < (1u << kh.l1bits); ++c) {
                kh.l2_tb0.push_back((uint32_t)tb + (c << (bb - kh.l1bits)));
                kh.l2_bits.push_back((bb << 8) | (bb - kh.l1bits));
            }
        tb += 1ull << bb;
        D2G_CHECK(ctx, tb < (1ull << 31), "--multiset: too many buckets in one batch; use smaller batches");
    }
    kh.gtab[2 * n] = (uint32_t)tb;
    kh.TB = (uint32_t)tb;
    kh.l2_start[n] = (uint32_t)kh.l2_tb0.size();
    kh.koff.assign(n + 1, 0);
    for (size_t g = 0; g < n; ++g) kh.koff[g + 1] = kh.koff[g] + kh.gk[g];
    // big inputs: buckets averaging more than K3_SPLIT_MIN keys are split once more (k3_split_kernel)
    // into sub-ranges of ~K3_TARGET keys; D2G_K3_SPLIT_MIN lowers the limit so that tests reach the path
    // (the compact path aims for 4x larger buckets -- 64-byte runs in the tile sort -- and always splits them here into
    // table-sized sub-ranges: a table round that re-reads its whole key range made the main pass 55 % slower, and a
    // bucket staged in LDS for the rounds cost more in occupancy than it saved: 42 ms instead of 20)
    const uint64_t split_min = t.split_min ? t.split_min : kh.compact ? K3_ROUND_KEYS : K3_SPLIT_MIN;
    kh.gsplit.assign(n, 0);
    kh.gsub.assign(n + 1, 0);
    for (size_t g = 0; g < n; ++g) {
        const uint64_t B = 1ull << kh.gtab[g], mean = kh.gk[g] / B;
        if (mean > split_min) {
            kh.gsplit[g] = std::min<uint32_t>(K3_MAXBBITS, ceil_log2((mean + t.sub_keys - 1) / t.sub_keys));
            kh.any_split = true;
        }
        // + 1: the end of a genome's last sub-range gets its OWN entry.  Sharing it with the next split genome's first
        // entry is only right when no unsplit genome lies between the two (their key ranges are then not adjacent and
        // the two writers race with different values)
        kh.gsub[g + 1] = kh.gsub[g] + (kh.gsplit[g] ? (B << kh.gsplit[g]) + 1 : 0);
    }
    return D2G_OK;
}

// registers and total weights (R12) / distinct (key, count) per bucket (R11) / their number only / One-Permutation registers over the
// k-mers counted at least thr + 1 times (K3o)
enum class K3Mode { Sketch, Count, Distinct, OphMin };

// count (R11) or sketch (R12) of one staged batch: what the caller fills in, the kernel arguments one stage prepares for the next, the stages
struct K3Run {
    d2g_ctx *ctx = nullptr; d2g_k3_state *st = nullptr; hipStream_t s = nullptr;
    KmerArgs km; size_t nblk = 0;      // the launch plan of the staged batch
    K3Host kh; size_t n = 0;           // its bucket layout (k3_layout); genomes
    uint64_t xormask = 0; size_t m = 1; double thr = 0.;
    uint64_t key_words = 0;            // d_keys in 8-byte words: a masked key per k-mer on the generic path, a 4-byte stored word on the compact one
    K3Args ka{}; K3cArgs kc{};         // bucket(): the generic / the compact form
    BmhArgs b{};                       // split, count, sketch
    uint64_t *oph_regs = nullptr;      // OphMin: the caller's registers [n][m] (device), pre-set to ~0 on this stream
    int run(K3Mode mode), upload_tables(), bucket_prepare(), bucket(size_t g_lo, size_t g_hi), split(), count(K3Mode mode), ophmin();
    int sketch(const std::vector<size_t> &sub), sketch_init(const std::vector<double> &guess), light_pass(const struct K3LightPlan &plan, bool pipeline);
    std::vector<size_t> subbatches(K3Mode mode) const;
    void init_registers() {            // registers to +inf, weights and redo flags to zero
        hipLaunchKernelGGL(k3_bmh_init_kernel, dim3((unsigned)div_up<size_t>(std::max<size_t>(n * m, n), K3_THREADS)), dim3(K3_THREADS), 0, s, st->d_h, n * m, st->d_tw, st->d_redo, n);
    }
};

// the tables every mode needs: bucket geometry and key offsets per genome, zeroed bucket counts and status
int K3Run::upload_tables() {
    const uint32_t TB = kh.TB;
    if (int rc = st->d_gtab.grow(ctx, 2 * n + 1, 4096)) return rc;
    if (int rc = st->d_bucket_cnt.grow(ctx, (size_t)TB + 1, 4096)) return rc;
    if (int rc = st->d_bucket_off.grow(ctx, (size_t)TB + 1, 4096)) return rc;
    if (int rc = st->d_cursor.grow(ctx, (size_t)TB + 1, 4096)) return rc;
    key_words = kh.compact ? (kh.total + 1) / 2 : kh.total;
    if (int rc = st->d_keys.grow(ctx, std::max<uint64_t>(key_words, 1), 4096)) return rc;
    if (!st->d_status) if (int rc = st->d_status.alloc(ctx, 2, "k3 status alloc")) return rc;
    if (int rc = st->d_koff.grow(ctx, n + 1, 4096)) return rc;
    D2G_HIP(ctx, hipMemcpyAsync(st->d_gtab, kh.gtab.data(), (2 * n + 1) * sizeof(uint32_t), hipMemcpyHostToDevice, s));
    D2G_HIP(ctx, hipMemcpyAsync(st->d_koff, kh.koff.data(), (n + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, s));
    D2G_HIP(ctx, hipMemsetAsync(st->d_bucket_cnt, 0, ((size_t)TB + 1) * sizeof(uint32_t), s));
    D2G_HIP(ctx, hipMemsetAsync(st->d_status, 0, 2 * sizeof(int), s));
    return D2G_OK;
}

// Sub-batch pipeline (generic path, sketching): the batch is cut into genome ranges; the bucketing passes of range j + 1
// (hist, scan, scatter, refine: bound by memory) run on the caller's stream while the counting pass of range j (bound by
// latency and instruction issue) runs on a second stream.  Ranges are independent: disjoint genomes, buckets, key regions.
// Returns the genome boundaries of the ranges; {0, n}: one range, no pipeline.
std::vector<size_t> K3Run::subbatches(K3Mode mode) const {
    std::vector<size_t> sub{0, n};
    if (kh.compact || kh.any_split || mode != K3Mode::Sketch || n < 2 || kh.gblk[n] != nblk) return sub;
    size_t want = ctx->k3_tune.subbatch ? ctx->k3_tune.subbatch : (n >= 8 && kh.total >= 200000000ull) ? 4 : 1;
    want = std::min(want, n);
    if (want == 1) return sub;
    sub.assign(1, 0);
    for (size_t j = 1; j < want; ++j) {                                  // cut by k-mer count
        const uint64_t target = kh.total / want * j;
        size_t g = sub.back() + 1;
        while (g < n - (want - j) && kh.koff[g] < target) ++g;
        sub.push_back(g);
    }
    sub.push_back(n);
    return sub;
}

// buffers, tables and kernel arguments of the bucketing passes
int K3Run::bucket_prepare() {
    if (kh.compact) {
        D2G_CHECK(ctx, kh.gblk[n] == nblk, "internal: K3 block layout disagrees with the launch plan");
        const size_t ntiles = std::max<size_t>(nblk * K1_CPT, 1);
        if (int rc = st->d_gblk.grow(ctx, n + 1, 4096)) return rc;
        if (int rc = st->d_tile_cnt.grow(ctx, ntiles * K3C_MAXB, 4096)) return rc;
        if (int rc = st->d_tile_off.grow(ctx, ntiles * K3C_MAXB, 4096)) return rc;
        D2G_HIP(ctx, hipMemcpyAsync(st->d_gblk, kh.gblk.data(), (n + 1) * sizeof(uint32_t), hipMemcpyHostToDevice, s));
        kc.km = km; kc.g_bbits = st->d_gtab; kc.g_boff = st->d_gtab + n; kc.g_koff = st->d_koff; kc.g_blk = st->d_gblk;
        kc.tile_cnt = st->d_tile_cnt; kc.tile_off = st->d_tile_off; kc.bucket_cnt = st->d_bucket_cnt; kc.bucket_off = st->d_bucket_off;
        kc.keys32 = reinterpret_cast<uint32_t *>(st->d_keys.get()); kc.hb = kh.hb; kc.TB = kh.TB;
        return D2G_OK;
    }
    K3Args &a = ka;
    a.km = km; a.xormask = xormask; a.g_bbits = st->d_gtab; a.g_boff = st->d_gtab + n; a.g_koff = st->d_koff;
    a.bucket_cnt = st->d_bucket_cnt; a.bucket_off = st->d_bucket_off; a.cursor = st->d_cursor; a.keys = st->d_keys;
    a.TB = kh.TB; a.l1bits = kh.l1bits; a.g0 = 0; a.n_genomes = (uint32_t)n;
    const size_t nl2 = kh.l2_tb0.size();
    if (nl2) {
        // the coarse keys borrow the sub-range buffer: k3_split_kernel (big inputs) runs after the refinement
        if (int rc = st->d_skeys.grow(ctx, std::max<uint64_t>(key_words, 1), 4096)) return rc;
        if (int rc = st->d_l2.grow(ctx, 2 * nl2, 4096)) return rc;
        D2G_HIP(ctx, hipMemcpyAsync(st->d_l2, kh.l2_tb0.data(), nl2 * sizeof(uint32_t), hipMemcpyHostToDevice, s));
        D2G_HIP(ctx, hipMemcpyAsync(st->d_l2 + nl2, kh.l2_bits.data(), nl2 * sizeof(uint32_t), hipMemcpyHostToDevice, s));
        a.coarse = st->d_skeys; a.l2_tb0 = st->d_l2; a.l2_bits = st->d_l2 + nl2;
    }
    if (int rc = st->d_blk_coarse.grow(ctx, std::max<size_t>(nblk, 1) << kh.l1bits, 4096)) return rc;
    a.blk_coarse = st->d_blk_coarse;
    return D2G_OK;
}
// the keys of genomes [g_lo, g_hi) into their buckets: hist -> scan -> scatter [-> refine].  The compact form (4-byte stored
// words, tile-sorted split: histogram per tile -> per-tile write offsets -> coalesced flush) takes the whole batch only.
int K3Run::bucket(size_t g_lo, size_t g_hi) {
    if (kh.compact) {
        const unsigned nb = (unsigned)nblk;
        const bool filt = km.ftab != nullptr;           // hist and scatter must drop the same k-mers: one switch for both
        const bool win = km.q > 1;                      // ... and walk the same ones: k-mers or minimizers
        const bool aa = d2g_km_protein(km);             // ... of the same alphabet (K1a: never with a window)
        const auto hist = aa ? (filt ? k3c_hist_kernel<true, false, true> : k3c_hist_kernel<false, false, true>)
                        : win ? (filt ? k3c_hist_kernel<true, true> : k3c_hist_kernel<false, true>) : (filt ? k3c_hist_kernel<true> : k3c_hist_kernel<false>);
        if (nb) hipLaunchKernelGGL(hist, dim3(nb), dim3(K1_THREADS), 0, s, kc);
        hipLaunchKernelGGL(k3c_scan_kernel, dim3((unsigned)n), dim3(K3_THREADS), 0, s, kc);
        if (nb) {
            const auto scatter = aa ? (filt ? k3c_scatter_kernel<true, false, true> : k3c_scatter_kernel<false, false, true>)
                               : win ? (filt ? k3c_scatter_kernel<true, true> : k3c_scatter_kernel<false, true>)
                                     : (filt ? k3c_scatter_kernel<true> : k3c_scatter_kernel<false>);
            D2G_HIP(ctx, hipFuncSetAttribute((const void *)scatter, hipFuncAttributeMaxDynamicSharedMemorySize, (int)sizeof(K3cScatterLds)));
            hipLaunchKernelGGL(scatter, dim3(nb), dim3(K1_THREADS), sizeof(K3cScatterLds), s, kc);
        }
        return D2G_OK;
    }
    K3Args a = ka;
    const unsigned blk_lo = kh.gblk[g_lo], nb = (g_lo == 0 && g_hi == n) ? (unsigned)nblk : kh.gblk[g_hi] - blk_lo;
    a.km.blk0 = blk_lo; a.g0 = (uint32_t)g_lo;
    const bool filt = km.ftab != nullptr;               // hist and scatter must drop the same k-mers: one switch for both
    const bool win = km.q > 1;                          // ... and walk the same ones: k-mers or minimizers
    const bool aa = d2g_km_protein(km);                 // ... of the same alphabet (K1a: never with a window)
    const auto hist = aa ? (filt ? k3_hist_kernel<true, false, true> : k3_hist_kernel<false, false, true>)
                    : win ? (filt ? k3_hist_kernel<true, true> : k3_hist_kernel<false, true>) : (filt ? k3_hist_kernel<true> : k3_hist_kernel<false>);
    const auto scatter = aa ? (filt ? k3_scatter_kernel<true, false, true> : k3_scatter_kernel<false, false, true>)
                       : win ? (filt ? k3_scatter_kernel<true, true> : k3_scatter_kernel<false, true>)
                             : (filt ? k3_scatter_kernel<true> : k3_scatter_kernel<false>);
    if (nb) hipLaunchKernelGGL(hist, dim3(nb), dim3(K1_THREADS), 0, s, a);
    hipLaunchKernelGGL(k3_scan_kernel, dim3((unsigned)(g_hi - g_lo)), dim3(K3_THREADS), 0, s, a);
    if (nb) hipLaunchKernelGGL(scatter, dim3(nb), dim3(K1_THREADS), 0, s, a);
    const unsigned l2_lo = kh.l2_start[g_lo], nl = kh.l2_start[g_hi] - l2_lo;
    if (nb && nl) {
        a.l2_tb0 += l2_lo; a.l2_bits += l2_lo;
        hipLaunchKernelGGL(k3_refine_kernel, dim3(nl), dim3(K3_THREADS), 0, s, a);
    }
    return D2G_OK;
}

// big inputs: the buckets of the genomes with gsplit[g] > 0 once more, into table-sized sub-ranges
int K3Run::split() {
    if (!kh.any_split) return D2G_OK;
    if (int rc = st->d_skeys.grow(ctx, std::max<uint64_t>(key_words, 1), 4096)) return rc;
    if (int rc = st->d_sub_off.grow(ctx, kh.gsub[n] + 1, 4096)) return rc;
    if (int rc = st->d_gsplit.grow(ctx, n, 4096)) return rc;
    if (int rc = st->d_gsub.grow(ctx, n + 1, 4096)) return rc;
    D2G_HIP(ctx, hipMemcpyAsync(st->d_gsplit, kh.gsplit.data(), n * sizeof(uint32_t), hipMemcpyHostToDevice, s));
    D2G_HIP(ctx, hipMemcpyAsync(st->d_gsub, kh.gsub.data(), (n + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, s));
    b.g_split = st->d_gsplit; b.g_sub = st->d_gsub; b.sub_off = st->d_sub_off; b.skeys = st->d_skeys;
    b.skeys32 = reinterpret_cast<uint32_t *>(st->d_skeys.get());
    const unsigned gs = (unsigned)std::min<size_t>(kh.TB, (size_t)ctx->num_cus * 8);
    hipLaunchKernelGGL(kh.compact ? k3_split_kernel<true> : k3_split_kernel<false>, dim3(gs), dim3(K3_THREADS), 0, s, b);
    return D2G_OK;
}

// R11 alone: the distinct (key, count) of every bucket -- K3Mode::Distinct: only how many -- stay in st->d_out_* / d_bucket_nd
int K3Run::count(K3Mode mode) {
    if (mode == K3Mode::Count) {
        if (int rc = st->d_out_keys.grow(ctx, std::max<uint64_t>(kh.total, 1), 4096)) return rc;
        if (int rc = st->d_out_counts.grow(ctx, std::max<uint64_t>(kh.total, 1), 4096)) return rc;
        b.out_keys = st->d_out_keys; b.out_counts = st->d_out_counts;
    }
    if (int rc = st->d_bucket_nd.grow(ctx, (size_t)kh.TB + 1, 4096)) return rc;
    b.bucket_nd = st->d_bucket_nd;
    if (kh.TB) hipLaunchKernelGGL(kh.compact ? k3_count_kernel<true> : k3_count_kernel<false>, dim3(kh.TB), dim3(K3_THREADS), 0, s, b);
    return D2G_OK;
}

// K3o: one workgroup per bucket, as count(); the registers are the caller's
int K3Run::ophmin() {
    b.h = oph_regs;
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
int K3Run::sketch_init(const std::vector<double> &guess) {
    const uint32_t TB = kh.TB;
    if (int rc = st->d_h.grow(ctx, std::max<size_t>(n * m, 1), 4096)) return rc;
    if (int rc = st->d_tw.grow(ctx, std::max<size_t>(n, 1), 4096)) return rc;
    if (int rc = st->d_guess.grow(ctx, std::max<size_t>(n, 1), 4096)) return rc;
    if (int rc = st->d_redo.grow(ctx, std::max<size_t>(n, 1), 4096)) return rc;
    if (int rc = st->d_tw_bucket.grow(ctx, (size_t)TB + 1, 4096)) return rc;
    D2G_HIP(ctx, hipMemsetAsync(st->d_tw_bucket, 0, ((size_t)TB + 1) * sizeof(double), s));
    D2G_HIP(ctx, hipMemcpyAsync(st->d_guess, guess.data(), n * sizeof(double), hipMemcpyHostToDevice, s));
    b.h = st->d_h; b.tw = st->d_tw; b.tw_acc = reinterpret_cast<uint64_t *>(st->d_tw_bucket.get()); b.guess = st->d_guess; b.redo = st->d_redo;
    b.nredo = reinterpret_cast<uint32_t *>(st->d_status + 1);
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
int K3Run::light_pass(const K3LightPlan &plan, bool pipeline) {
    if (pipeline && !st->xs) {
        D2G_HIP(ctx, st->xs.create(hipStreamNonBlocking));
        for (auto &e : st->ev_a) D2G_HIP(ctx, e.create(hipEventDisableTiming));
        D2G_HIP(ctx, st->ev_b.create(hipEventDisableTiming));
    }
    hipStream_t xs = pipeline ? (hipStream_t)st->xs : s;
    for (size_t j = 0; j < (pipeline ? plan.ll.size() : 1); ++j) {
        const LightLaunch &L = plan.ll[j];
        BmhArgs x = b;
        x.tb0 = L.t0; x.tb1 = L.t1; x.g0 = L.g0; x.redo_mode = 0;
        x.gq = reinterpret_cast<QEntry *>(st->d_gq.get()) + L.entry0;
        x.gq_off = st->d_gq_off + L.off_at;
        x.gq_n = reinterpret_cast<uint32_t *>(st->d_gq_off.get()) + L.n_at;
        if (pipeline) {
            if (int rc = bucket(L.g0, L.g1)) return rc;
            D2G_HIP(ctx, hipEventRecord(st->ev_a[j], s));
            D2G_HIP(ctx, hipStreamWaitEvent(xs, st->ev_a[j], 0));
        }
        if (!pipeline || L.t1 > L.t0) {
            hipLaunchKernelGGL(k3_main_kernel(kh.compact, true), dim3(L.grid), dim3(K3_THREADS), 0, xs, x);
            hipLaunchKernelGGL(k3_bmh_survivor_kernel, dim3(L.grid), dim3(K3_THREADS), 0, xs, x);
        }
        if (pipeline) hipLaunchKernelGGL(k3_bmh_verify_kernel, dim3(L.g1 - L.g0), dim3(K3_THREADS), 0, xs, x);
        else hipLaunchKernelGGL(k3_bmh_verify_kernel, dim3((unsigned)n), dim3(K3_THREADS), 0, s, b);
    }
    if (pipeline) {
        D2G_HIP(ctx, hipEventRecord(st->ev_b, xs));
        D2G_HIP(ctx, hipStreamWaitEvent(s, st->ev_b, 0));
    }
    return D2G_OK;
}

// R12: registers and total weights of the bucketed batch stay in st->d_h / st->d_tw.  `sub`: subbatches()
int K3Run::sketch(const std::vector<size_t> &sub) {
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
    if (pipeline && !light) { if (int rc = bucket(0, n)) return rc; pipeline = false; }   // heavy first pass: one range
    K3LightPlan plan;
    if (light) {
        plan = k3_plan_light(kh, t, guess, ctx->num_cus, sub);
        if (int rc = st->d_gq.grow(ctx, (size_t)plan.entries * (sizeof(QEntry) / 8) + 8, 4096)) return rc;
        if (int rc = st->d_gq_off.grow(ctx, plan.off.size() + (plan.n_words + 1) / 2 + 1, 4096)) return rc;
        D2G_HIP(ctx, hipMemcpyAsync(st->d_gq_off, plan.off.data(), plan.off.size() * sizeof(uint64_t), hipMemcpyHostToDevice, s));
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
        D2G_HIP(ctx, hipMemcpyAsync(st2, st->d_status, sizeof(st2), hipMemcpyDeviceToHost, s));
        D2G_HIP(ctx, hipStreamSynchronize(s));
        if (pass == FirstLight && st2[0] == K3_REGION_OVERFLOW) {
            D2G_HIP(ctx, hipMemsetAsync(st->d_status, 0, 2 * sizeof(int), s));
            D2G_HIP(ctx, hipMemsetAsync(st->d_tw_bucket, 0, ((size_t)TB + 1) * sizeof(double), s));
            init_registers();
            pass = FirstHeavy;
            continue;
        }
        if (st2[0] || !st2[1]) break;
        D2G_CHECK(ctx, redos < 40, "internal: BagMinHash bound did not converge");
        ++redos; pass = Redo;
        D2G_HIP(ctx, hipMemsetAsync(st->d_status + 1, 0, sizeof(int), s));
    }
    return D2G_OK;
}

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
    b.keys = st->d_keys; b.keys32 = reinterpret_cast<const uint32_t *>(st->d_keys.get()); b.g_bbits = st->d_gtab; b.hb = kh.hb; b.xormask = xormask;
    b.bucket_off = st->d_bucket_off; b.g_boff = st->d_gtab + n;
    b.n = (uint32_t)n; b.TB = kh.TB; b.m = (uint32_t)m; b.thr = thr; b.status = st->d_status; b.round_keys = ctx->k3_tune.round_keys;
    if (int rc = split()) return rc;
    if (int rc = mode == K3Mode::Sketch ? sketch(sub) : mode == K3Mode::OphMin ? ophmin() : count(mode)) return rc;
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
    D2G_HIP(ctx, hipMemcpyAsync(&status, st->d_status, sizeof(int), hipMemcpyDeviceToHost, s));
    D2G_HIP(ctx, hipStreamSynchronize(s));
    return k3_status_error(ctx, status);
}

// what every K3 operation begins with: the work state of the batch's owner (made on first use), the run filled from the batch, the
// bucket layout.  The only place that fills a K3Run's ctx / st / s / n / km / nblk.
int k3_begin(const KmerBatch &b, K3Run &r) {
    if (!*b.k3) *b.k3 = new (std::nothrow) d2g_k3_state();
    if (!*b.k3) return D2G_ERR_NOMEM;
    r.ctx = b.ctx; r.st = *b.k3; r.s = b.s; r.n = b.runs.n; r.km = b.km; r.nblk = b.nblk;
    return k3_layout(b.ctx, b.runs, r.kh);
}

// BagMinHash.  The checks stand in front of the batch (a stage uploads; a refusal comes before it); the operation leaves registers
// [n][sketchsize] and total weights [n] in the state and copies them out as `out` says: device to host or device to device
int bmh_check(d2g_ctx *ctx, size_t n, size_t sketchsize, double count_threshold, const double *sig_out, const double *total_weight_out) {
    D2G_CHECK(ctx, sketchsize >= 1 && sketchsize < (1ull << 24), "sketchsize out of range");
    D2G_CHECK(ctx, (sig_out && total_weight_out) || n == 0, "null output");
    D2G_CHECK(ctx, count_threshold == count_threshold, "count_threshold is NaN");
    return D2G_OK;
}
int bmh_sketch(const KmerBatch &b, uint64_t xormask, size_t sketchsize, double count_threshold, double *sig_out, double *total_weight_out,
               hipMemcpyKind out) {
    d2g_ctx *ctx = b.ctx;
    K3Run r;
    if (int rc = k3_begin(b, r)) return rc;
    const size_t n = r.n;
    if (n == 0) return D2G_OK;
    r.xormask = xormask; r.m = sketchsize; r.thr = count_threshold;
    if (int rc = r.run(K3Mode::Sketch)) return rc;
    D2G_HIP(ctx, hipMemcpyAsync(sig_out, r.st->d_h, n * sketchsize * sizeof(double), out, r.s));
    D2G_HIP(ctx, hipMemcpyAsync(total_weight_out, r.st->d_tw, n * sizeof(double), out, r.s));
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
    D2G_HIP(ctx, hipMemcpyAsync(nd.data(), r.st->d_bucket_nd, kh.TB * sizeof(uint32_t), hipMemcpyDeviceToHost, r.s));
    D2G_HIP(ctx, hipStreamSynchronize(r.s));
    for (size_t g = 0; g < n; ++g) {
        uint64_t t = 0;
        for (uint32_t tb = kh.gtab[n + g]; tb < kh.gtab[n + g + 1]; ++tb) t += nd[tb];
        ndistinct_out[g] = t;
    }
    return D2G_OK;
}

// the exact (key, count) of every bucket of a begun run (n > 0), left in the state: what the count and both set forms read
int k3_exact_counts(K3Run &r, uint64_t xormask, double count_threshold) {
    r.xormask = xormask; r.thr = count_threshold;
    if (int rc = r.run(K3Mode::Count)) return rc;
    return k3_check_status(r.ctx, r.st, r.s);
}

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
    D2G_HIP(ctx, hipMemcpy(nd.data(), st->d_bucket_nd, kh.TB * sizeof(uint32_t), hipMemcpyDeviceToHost));
    D2G_HIP(ctx, hipMemcpy(boff.data(), st->d_bucket_off, ((size_t)kh.TB + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost));
    if (kh.total) {
        D2G_HIP(ctx, hipMemcpy(hk.data(), st->d_out_keys, kh.total * sizeof(uint64_t), hipMemcpyDeviceToHost));
        D2G_HIP(ctx, hipMemcpy(hc.data(), st->d_out_counts, kh.total * sizeof(uint32_t), hipMemcpyDeviceToHost));
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

// ---- K3s: the exact sets in SORTED form, on the device (Counter::finalize(vector&, vector&, thr) WITH its sort, src/counter.h:78-117)
// k3_count_kernel leaves the distinct (key, count) of every K3 bucket at the front of the bucket's region, in table order.  The bucket
// index is the key's top bits on the generic path only (the compact path's k3c_bucket is another mapping, and sub-ranges and table
// rounds reorder inside a bucket on both), so the emission does not lean on it: it is a segmented sort of its own, MSD first.
//   ks_hist     every element counts into sort range (genome, top pbits[g] bits of the key); pbits[g] aims at sort_keys (1024) keys
//               per range from the genome's k-mer count, an upper bound of its distinct count; sums the counts per genome
//   ks_scan     one workgroup: exclusive prefix over all ranges = where each range, and with it each set, begins in the output
//   ks_scatter  every element to a slot of its range (one cursor per range)
//   ks_sort     one workgroup per range: bitonic sort of (key, count) in LDS, written back in place
// Ranges ascend with the key inside a genome, so a genome's slice ends strictly ascending.  Keys are Wang hashes: a range of mean
// <= 1024 keys never reaches the 2048 the LDS stage takes (32 standard deviations); keys that do (not hashes) end in K3_SORT_OVERFLOW, reported, never silent.
constexpr int KS_SORT_CAP = 2048;            // keys of one sort range in LDS: 24 KiB with the counts, six workgroups per CU
constexpr int KS_SCAN_THREADS = 1024;

struct KsArgs {
    const uint64_t *src_keys; const uint32_t *src_counts;      // k3_count_kernel's output, bucket by bucket
    const uint64_t *bucket_off; const uint32_t *bucket_nd; const uint32_t *g_boff;
    uint32_t n, TB;
    const uint32_t *g_pbits;     // [n]
    const uint64_t *g_rbase;     // [n+1]
    uint64_t nranges;
    uint32_t *range_cnt;         // [nranges], zeroed
    uint64_t *range_off;         // [nranges+1]
    uint64_t *cursor;            // [nranges]
    uint64_t *keys; uint32_t *counts;                          // the output; ks_sort sorts it in place
    uint64_t *set_off;           // [n+1]
    uint64_t *cards;             // [n][2]: distinct keys, sum of the counts (zeroed; ks_hist adds the sums)
    int *status;
};

__device__ __forceinline__ uint64_t ks_range_of(const KsArgs &a, uint32_t g, uint64_t key) {
    const uint32_t pb = a.g_pbits[g];
    return a.g_rbase[g] + (pb ? key >> (64 - pb) : 0ull);
}

// Lanes of a wave that fall into the same sort range share ONE atomic (the first of them adds their number; with a cursor, each takes
// its rank behind the returned base): on the generic path a K3 bucket lies inside one or two sort ranges, so a wave issues one or two
// atomics instead of 64 on one address.  The loop is uniform over the wave (`todo` is a ballot).
template <bool SCATTER>
__global__ __launch_bounds__(K3_THREADS) void ks_place_kernel(KsArgs a) {
    const uint32_t tb = blockIdx.x;
    const uint32_t nd = a.bucket_nd[tb];
    if (nd == 0) return;
    const uint64_t o0 = a.bucket_off[tb];
    const uint32_t g = genome_of_bucket(a.g_boff, a.n, tb);
    const uint32_t lane = threadIdx.x & 63;
    uint64_t csum = 0;
    for (uint32_t e0 = 0; e0 < nd; e0 += K3_THREADS) {
        const uint32_t e = e0 + threadIdx.x;
        const bool have = e < nd;
        uint64_t key = 0, r = 0, pos = 0;
        uint32_t c = 0;
        if (have) { key = a.src_keys[o0 + e]; c = a.src_counts[o0 + e]; r = ks_range_of(a, g, key); }
        unsigned long long todo = __ballot(have);
        while (todo) {
            const int leader = __ffsll((long long)todo) - 1;
            const uint64_t r0 = __shfl((unsigned long long)r, leader);
            const bool mine = have && r == r0;
            const unsigned long long same = __ballot(mine);
            const uint32_t cnt = (uint32_t)__popcll(same);
            if constexpr (SCATTER) {
                unsigned long long base = 0;
                if ((int)lane == leader) base = atomicAdd((unsigned long long *)&a.cursor[r0], (unsigned long long)cnt);
                base = __shfl(base, leader);
                if (mine) pos = base + (uint32_t)__popcll(same & ((1ull << lane) - 1ull));
            } else if ((int)lane == leader) atomicAdd(&a.range_cnt[r0], cnt);
            todo &= ~same;
        }
        if constexpr (SCATTER) { if (have) { a.keys[pos] = key; a.counts[pos] = c; } }
        else csum += c;
    }
    if constexpr (!SCATTER) {
        __shared__ unsigned long long sum;
        if (threadIdx.x == 0) sum = 0;
        __syncthreads();
        if (csum) atomicAdd(&sum, (unsigned long long)csum);
        __syncthreads();
        if (threadIdx.x == 0 && sum) atomicAdd((unsigned long long *)&a.cards[2 * (size_t)g + 1], sum);
    }
}

__global__ __launch_bounds__(KS_SCAN_THREADS) void ks_scan_kernel(KsArgs a) {
    __shared__ uint64_t part[KS_SCAN_THREADS];
    __shared__ uint64_t running;
    const int tid = threadIdx.x;
    if (tid == 0) running = 0;
    __syncthreads();
    for (uint64_t base = 0; base < a.nranges; base += KS_SCAN_THREADS) {
        const uint64_t i = base + tid;
        const uint64_t v = i < a.nranges ? a.range_cnt[i] : 0u;
        part[tid] = v;
        __syncthreads();
        for (int d = 1; d < KS_SCAN_THREADS; d <<= 1) {          // inclusive Hillis-Steele prefix
            const uint64_t x = tid >= d ? part[tid - d] : 0;
            __syncthreads();
            part[tid] += x;
            __syncthreads();
        }
        const uint64_t off = running + part[tid] - v;
        if (i < a.nranges) { a.range_off[i] = off; a.cursor[i] = off; }
        __syncthreads();
        if (tid == KS_SCAN_THREADS - 1) running += part[tid];
        __syncthreads();
    }
    if (tid == 0) a.range_off[a.nranges] = running;
    __syncthreads();
    for (uint32_t g = tid; g <= a.n; g += KS_SCAN_THREADS) {
        const uint64_t o = a.range_off[a.g_rbase[g]];
        a.set_off[g] = o;
        if (g < a.n) a.cards[2 * (size_t)g] = a.range_off[a.g_rbase[g + 1]] - o;
    }
}

// (key, count) order of the sort: by key; a pad (key ~0, count 0) after a real element of key ~0 (real counts are >= 1)
__device__ __forceinline__ bool ks_before(uint64_t ka, uint32_t ca, uint64_t kb, uint32_t cb) { return ka < kb || (ka == kb && ca > cb); }

__global__ __launch_bounds__(K3_THREADS) void ks_sort_kernel(KsArgs a) {
    __shared__ uint64_t key[KS_SORT_CAP];
    __shared__ uint32_t cnt[KS_SORT_CAP];
    const uint64_t r = blockIdx.x;
    const uint64_t o0 = a.range_off[r], nk = a.range_off[r + 1] - o0;
    if (nk < 2) return;
    if (nk > KS_SORT_CAP) { if (threadIdx.x == 0) atomicExch(a.status, K3_SORT_OVERFLOW); return; }
    uint32_t np2 = 2;
    while (np2 < nk) np2 <<= 1;
    for (uint32_t i = threadIdx.x; i < np2; i += K3_THREADS) {
        key[i] = i < nk ? a.keys[o0 + i] : ~0ull;
        cnt[i] = i < nk ? a.counts[o0 + i] : 0u;
    }
    __syncthreads();
    for (uint32_t k = 2; k <= np2; k <<= 1)
        for (uint32_t j = k >> 1; j > 0; j >>= 1) {
            for (uint32_t t = threadIdx.x; t < np2 / 2; t += K3_THREADS) {       // one compare-exchange per thread and turn: no idle half
                const uint32_t i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), p = i | j;
                const uint64_t ka = key[i], kb = key[p];
                const uint32_t ca = cnt[i], cb = cnt[p];
                const bool up = (i & k) == 0;
                if (up ? ks_before(kb, cb, ka, ca) : ks_before(ka, ca, kb, cb)) { key[i] = kb; key[p] = ka; cnt[i] = cb; cnt[p] = ca; }
            }
            __syncthreads();
        }
    for (uint32_t i = threadIdx.x; i < nk; i += K3_THREADS) { a.keys[o0 + i] = key[i]; a.counts[o0 + i] = cnt[i]; }
}

// After r.run(K3Mode::Count) and its status check: the sets of the staged batch, sorted, into keys_dev / counts_dev (cap entries each;
// counts_dev may be null), set_off_dev [n+1] and cards_dev [n][2].  Waits for the total before it writes any of them: a cap that is
// too small is D2G_ERR_INVALID with every output untouched.  Waits again for the status word.  *total_out: entries written.
int k3_sorted_sets(K3Run &r, const char *who, uint64_t *keys_dev, uint32_t *counts_dev, size_t cap, uint64_t *set_off_dev,
                   uint64_t *cards_dev, uint64_t *total_out) {
    d2g_ctx *ctx = r.ctx; d2g_k3_state *st = r.st; hipStream_t s = r.s;
    const K3Host &kh = r.kh;
    const size_t n = r.n;
    const uint64_t target = ctx->k3_tune.sort_keys;
    std::vector<uint32_t> pbits(n);
    std::vector<uint64_t> rbase(n + 1, 0);
    for (size_t g = 0; g < n; ++g) {
        pbits[g] = std::min<uint32_t>(32, ceil_log2((kh.gk[g] + target - 1) / target));
        rbase[g + 1] = rbase[g] + (1ull << pbits[g]);
    }
    const uint64_t nranges = rbase[n];
    D2G_CHECK(ctx, nranges < (1ull << 31), "exact k-mer sets: too many sort ranges in one batch; use smaller batches");
    if (int rc = st->d_ks_pbits.grow(ctx, n, 4096)) return rc;
    if (int rc = st->d_ks_rbase.grow(ctx, n + 1, 4096)) return rc;
    if (int rc = st->d_ks_cnt.grow(ctx, nranges, 4096)) return rc;
    if (int rc = st->d_ks_off.grow(ctx, nranges + 1, 4096)) return rc;
    if (int rc = st->d_ks_cur.grow(ctx, nranges, 4096)) return rc;
    if (int rc = st->d_ks_setoff.grow(ctx, n + 1, 4096)) return rc;
    if (int rc = st->d_ks_cards.grow(ctx, 2 * n, 4096)) return rc;
    D2G_HIP(ctx, hipMemcpyAsync(st->d_ks_pbits, pbits.data(), n * sizeof(uint32_t), hipMemcpyHostToDevice, s));
    D2G_HIP(ctx, hipMemcpyAsync(st->d_ks_rbase, rbase.data(), (n + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, s));
    D2G_HIP(ctx, hipMemsetAsync(st->d_ks_cnt, 0, nranges * sizeof(uint32_t), s));
    D2G_HIP(ctx, hipMemsetAsync(st->d_ks_cards, 0, 2 * n * sizeof(uint64_t), s));
    KsArgs a{};
    a.src_keys = st->d_out_keys; a.src_counts = st->d_out_counts; a.bucket_off = st->d_bucket_off; a.bucket_nd = st->d_bucket_nd;
    a.g_boff = st->d_gtab + n; a.n = (uint32_t)n; a.TB = kh.TB; a.g_pbits = st->d_ks_pbits; a.g_rbase = st->d_ks_rbase; a.nranges = nranges;
    a.range_cnt = st->d_ks_cnt; a.range_off = st->d_ks_off; a.cursor = st->d_ks_cur; a.set_off = st->d_ks_setoff; a.cards = st->d_ks_cards;
    a.status = st->d_status;
    d2g_timer tm(ctx, &ctx->ev_k3s, s);
    if (kh.TB) hipLaunchKernelGGL(ks_place_kernel<false>, dim3(kh.TB), dim3(K3_THREADS), 0, s, a);
    hipLaunchKernelGGL(ks_scan_kernel, dim3(1), dim3(KS_SCAN_THREADS), 0, s, a);
    uint64_t total = 0;
    D2G_HIP(ctx, hipMemcpyAsync(&total, st->d_ks_off + nranges, sizeof(uint64_t), hipMemcpyDeviceToHost, s));
    D2G_HIP(ctx, hipStreamSynchronize(s));
    if (total > cap) {
        tm.stop();
        char msg[160];
        std::snprintf(msg, sizeof msg, "%s: output capacity too small (%llu entries needed, cap %llu)", who, (unsigned long long)total,
                      (unsigned long long)cap);
        ctx->last_error = msg;
        return D2G_ERR_INVALID;
    }
    if (total_out) *total_out = total;
    if (!counts_dev && total) {                                  // the sort's tie rule reads the counts: keys alone get a private column
        if (int rc = st->d_ks_counts.grow(ctx, total, 4096)) return rc;
        counts_dev = st->d_ks_counts;
    }
    a.keys = keys_dev; a.counts = counts_dev;
    if (kh.TB && total) {
        hipLaunchKernelGGL(ks_place_kernel<true>, dim3(kh.TB), dim3(K3_THREADS), 0, s, a);
        hipLaunchKernelGGL(ks_sort_kernel, dim3((unsigned)nranges), dim3(K3_THREADS), 0, s, a);
    }
    tm.stop();
    D2G_HIP(ctx, hipGetLastError());
    D2G_HIP(ctx, hipMemcpyAsync(set_off_dev, st->d_ks_setoff, (n + 1) * sizeof(uint64_t), hipMemcpyDeviceToDevice, s));
    D2G_HIP(ctx, hipMemcpyAsync(cards_dev, st->d_ks_cards, 2 * n * sizeof(uint64_t), hipMemcpyDeviceToDevice, s));
    return k3_check_status(ctx, st, s);
}

// the checks of both forms of the exact sets, in front of the batch; `sfx` names the form's outputs in the refusal ("out", "dev")
int sets_check(d2g_ctx *ctx, size_t n, double count_threshold, const uint64_t *keys, size_t cap, const uint64_t *set_off, const uint64_t *cards,
               const char *sfx) {
    D2G_CHECK(ctx, set_off != nullptr, std::string("null set_off_") + sfx);
    D2G_CHECK(ctx, cards != nullptr || n == 0, std::string("null cards_") + sfx);
    D2G_CHECK(ctx, cap == 0 || keys, "null output");
    D2G_CHECK(ctx, count_threshold == count_threshold, "count_threshold is NaN");
    return D2G_OK;
}

// the device form: k3_sorted_sets straight into the caller's arrays
int kmer_sets_dev(const KmerBatch &b, uint64_t xormask, double count_threshold, uint64_t *keys_dev, uint32_t *counts_dev, size_t cap,
                  uint64_t *set_off_dev, uint64_t *cards_dev) {
    K3Run r;
    if (int rc = k3_begin(b, r)) return rc;
    if (r.n == 0) {
        D2G_HIP(b.ctx, hipMemsetAsync(set_off_dev, 0, sizeof(uint64_t), r.s));
        return D2G_OK;
    }
    if (int rc = k3_exact_counts(r, xormask, count_threshold)) return rc;
    return k3_sorted_sets(r, "d2g_kmer_sets_dev", keys_dev, counts_dev, cap, set_off_dev, cards_dev, nullptr);
}

// the host-pointer form: that function on the sketcher's own buffers, then copied out
int sketcher_kmer_sets(d2g_sketcher *sk, const PackedRuns &in, uint64_t xormask, double count_threshold, uint64_t *keys_out,
                       uint32_t *counts_out, size_t cap, uint64_t *set_off_out, uint64_t *cards_out) {
    if (!sk) return D2G_ERR_INVALID;
    d2g_ctx *ctx = sk->ctx;
    const size_t n = in.n;
    if (int rc = sets_check(ctx, n, count_threshold, keys_out, cap, set_off_out, cards_out, "out")) return rc;
    KmerBatch b;
    if (int rc = d2g_sketcher_stage(sk, in, &b, nullptr)) return rc;
    K3Run r;
    if (int rc = k3_begin(b, r)) return rc;
    d2g_k3_state *st = r.st;
    if (n == 0) { set_off_out[0] = 0; return D2G_OK; }
    if (int rc = k3_exact_counts(r, xormask, count_threshold)) return rc;
    const uint64_t room = std::max<uint64_t>(r.kh.total, 1);
    if (int rc = st->d_ks_keys.grow(ctx, room, 4096)) return rc;
    if (int rc = st->d_ks_counts.grow(ctx, room, 4096)) return rc;
    d2g_dev<uint64_t> d_meta;                                    // set_off [n+1], cards [n][2]
    if (int rc = d_meta.alloc(ctx, 3 * n + 1, "exact k-mer sets: offsets")) return rc;
    uint64_t total = 0;
    if (int rc = k3_sorted_sets(r, "d2g_kmer_sets", st->d_ks_keys, st->d_ks_counts, std::min<uint64_t>(cap, room), d_meta, d_meta + n + 1, &total))
        return rc;
    if (total) {
        D2G_HIP(ctx, hipMemcpyAsync(keys_out, st->d_ks_keys, total * sizeof(uint64_t), hipMemcpyDeviceToHost, r.s));
        if (counts_out) D2G_HIP(ctx, hipMemcpyAsync(counts_out, st->d_ks_counts, total * sizeof(uint32_t), hipMemcpyDeviceToHost, r.s));
    }
    D2G_HIP(ctx, hipMemcpyAsync(set_off_out, d_meta, (n + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost, r.s));
    D2G_HIP(ctx, hipMemcpyAsync(cards_out, d_meta + n + 1, 2 * n * sizeof(uint64_t), hipMemcpyDeviceToHost, r.s));
    D2G_HIP(ctx, hipStreamSynchronize(r.s));
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

int d2g_kmer_sets(d2g_ctx *ctx, const uint8_t *packed, size_t packed_bytes, const uint64_t *run_start,
                  const uint32_t *run_len, size_t nrun, const uint64_t *genome_run_off, size_t n, int k, int canon,
                  uint64_t xormask, double count_threshold, uint64_t *keys_out, uint32_t *counts_out, size_t cap,
                  uint64_t *set_off_out, uint64_t *cards_out) {
    const PackedRuns in{packed, packed_bytes, run_start, run_len, nrun, genome_run_off, n, k, canon};
    return d2g_with_sketcher(ctx, [&](d2g_sketcher *sk) {
        return sketcher_kmer_sets(sk, in, xormask, count_threshold, keys_out, counts_out, cap, set_off_out, cards_out);
    });
}

int d2g_sketcher_run_sets(d2g_sketcher *sk, const uint8_t *packed, size_t packed_bytes, const uint64_t *run_start, const uint32_t *run_len,
                          size_t nrun, const uint64_t *genome_run_off, size_t n, int k, int canon, uint64_t xormask, double count_threshold,
                          uint64_t *keys_out, uint32_t *counts_out, size_t cap, uint64_t *set_off_out, uint64_t *cards_out) {
    const PackedRuns in{packed, packed_bytes, run_start, run_len, nrun, genome_run_off, n, k, canon};
    return sketcher_kmer_sets(sk, in, xormask, count_threshold, keys_out, counts_out, cap, set_off_out, cards_out);
}

int d2g_kmer_sets_dev(d2g_ctx *ctx, const d2g_oph_plan *plan, const uint8_t *packed_dev, int canon, uint64_t xormask,
                      double count_threshold, uint64_t *keys_dev, uint32_t *counts_dev, size_t cap, uint64_t *set_off_dev,
                      uint64_t *cards_dev, void *stream) {
    if (!ctx || !plan) return D2G_ERR_INVALID;
    if (int rc = sets_check(ctx, plan->n, count_threshold, keys_dev, cap, set_off_dev, cards_dev, "dev")) return rc;
    KmerBatch b;
    if (int rc = d2g_plan_batch(ctx, plan, packed_dev, canon, stream, &b)) return rc;
    return kmer_sets_dev(b, xormask, count_threshold, keys_dev, counts_dev, cap, set_off_dev, cards_dev);
}

// Every host-side check of the weights of explicit sets, without a context.  The last one keeps the walk finite: a set's first guess of
// its bound is scale * bmh_guess(W), the redo loop of d2g_bmh_from_weighted_ids multiplies a guess by 16 and gives up after 40 passes, so
// a first guess below 2^1024 / 16^40 = 2^864 stays finite through every pass.  An infinite bound prunes nothing (proc_next ends on
// P.x <= bound, which inf <= inf satisfies), and the walk of such a set would not end.
constexpr double BMH_GUESS_LIMIT = 0x1p864;
int d2g_bmh_check_weights(const double *weights, const uint64_t *set_off, size_t nsets, size_t sketchsize, double scale, char *err,
                          size_t errcap) {
    auto fail = [&](const char *fmt, unsigned long long set) {
        if (err && errcap) std::snprintf(err, errcap, fmt, set);
        return D2G_ERR_INVALID;
    };
    if (err && errcap) err[0] = 0;
    if (!set_off) return fail("null argument", 0);
    if (!(sketchsize >= 1 && sketchsize < (1ull << 24))) return fail("sketchsize out of range", 0);
    if (!(scale > 0.)) return fail("guess scale not positive", 0);
    for (size_t i = 0; i < nsets; ++i) if (!(set_off[i] <= set_off[i + 1])) return fail("set_off not monotone", 0);
    const double m = (double)sketchsize, lnm = std::log(m);
    for (size_t i = 0; i < nsets; ++i) {
        double t = 0.;
        for (uint64_t e = set_off[i]; e < set_off[i + 1]; ++e) {
            const double w = weights ? weights[e] : 1.0;
            if (w > 0.) {
                if (!(w <= 0x1p53)) return fail("BagMinHash weight outside (0, 2^53] (set %llu)", i);
                t += w;
            } else if (w != w) return fail("BagMinHash weight is NaN (set %llu)", i);
        }
        if (t > 0. && !(scale * bmh_guess(t, m, lnm) < BMH_GUESS_LIMIT))
            return fail("BagMinHash set %llu: total weight too small for the sketch size (the pruning bound would not stay finite)", i);
    }
    return D2G_OK;
}

int d2g_bmh_from_weighted(d2g_ctx *ctx, const uint64_t *ids, const double *weights, const uint64_t *set_off, size_t nsets,
                          size_t sketchsize, double *sig_out, double *total_weight_out) {
    return d2g_bmh_from_weighted_ids(ctx, ids, weights, set_off, nsets, sketchsize, sig_out, total_weight_out, nullptr);
}

int d2g_bmh_from_weighted_ids(d2g_ctx *ctx, const uint64_t *ids, const double *weights, const uint64_t *set_off, size_t nsets,
                              size_t sketchsize, double *sig_out, double *total_weight_out, uint64_t *owner_out) {
    if (!ctx) return D2G_ERR_INVALID;
    D2G_CHECK(ctx, set_off != nullptr && (nsets == 0 || (sig_out && total_weight_out)), "null argument");
    D2G_CHECK(ctx, sketchsize >= 1 && sketchsize < (1ull << 24), "sketchsize out of range");
    D2G_CHECK(ctx, nsets < (1ull << 31), "too many sets");
    if (nsets == 0) return D2G_OK;
    const uint64_t total = set_off[nsets];
    D2G_CHECK(ctx, total == 0 || ids != nullptr, "null ids");
    {   // every check of the weights, before anything is allocated or launched
        char err[160];
        if (d2g_bmh_check_weights(weights, set_off, nsets, sketchsize, ctx->k3_tune.guess_scale, err, sizeof err) != D2G_OK) {
            ctx->last_error = err;
            return D2G_ERR_INVALID;
        }
    }
    D2G_HIP(ctx, hipSetDevice(ctx->device));
    const size_t m = sketchsize;
    // total weights on the host (the caller's arrays are host arrays): the result, and the first guess of the bound
    std::vector<double> tw(nsets, 0.);
    for (size_t i = 0; i < nsets; ++i) {
        const uint64_t lo = set_off[i], hi = set_off[i + 1];
        double t = 0.;
        for (uint64_t e = lo; e < hi; ++e) {
            const double w = weights ? weights[e] : 1.0;
            if (w > 0.) t += w;                                      // the same sum, in the same order, as d2g_bmh_check_weights
        }
        tw[i] = t;
    }
    const std::vector<uint64_t> guess = ws_guesses(tw.data(), nsets, m, ctx->k3_tune.guess_scale);
    d2g_ws_blocks wb;
    d2g_ws_plan_blocks(set_off, nsets, wb);
    const std::vector<uint32_t> &bset = wb.set, &bcnt = wb.cnt;
    const std::vector<uint64_t> &blo = wb.lo;
    D2G_CHECK(ctx, bset.size() < (1ull << 31), "too many workgroups");
    const size_t nb = bset.size();
    d2g_dev<uint64_t> d_ids, d_blo, d_h, d_guess, d_arg, d_setlo;
    d2g_dev<double> d_w, d_tw;
    d2g_dev<uint32_t> d_bset, d_bcnt, d_redo;
    d2g_dev<int> d_status;
    int rc = D2G_OK;
    const char *what = "weighted sets alloc";
    if ((rc = d_ids.alloc(ctx, std::max<uint64_t>(total, 1), what)) ||
        (rc = d_blo.alloc(ctx, std::max<size_t>(nb, 1), what)) ||
        (rc = d_bset.alloc(ctx, std::max<size_t>(nb, 1), what)) ||
        (rc = d_bcnt.alloc(ctx, std::max<size_t>(nb, 1), what)) ||
        (rc = d_h.alloc(ctx, nsets * m, what)) ||
        (rc = d_guess.alloc(ctx, nsets, what)) ||
        (rc = d_redo.alloc(ctx, nsets, what)) ||
        (rc = d_tw.alloc(ctx, nsets, what)) ||
        (rc = d_status.alloc(ctx, 2, what))) return rc;
    if (weights) { if ((rc = d_w.alloc(ctx, std::max<uint64_t>(total, 1), what))) return rc; D2G_HIP(ctx, hipMemcpy(d_w, weights, total * 8, hipMemcpyHostToDevice)); }
    if (total) D2G_HIP(ctx, hipMemcpy(d_ids, ids, total * 8, hipMemcpyHostToDevice));
    D2G_HIP(ctx, hipMemcpy(d_guess, guess.data(), nsets * 8, hipMemcpyHostToDevice));
    if (nb) {
        D2G_HIP(ctx, hipMemcpy(d_blo, blo.data(), nb * 8, hipMemcpyHostToDevice));
        D2G_HIP(ctx, hipMemcpy(d_bset, bset.data(), nb * 4, hipMemcpyHostToDevice));
        D2G_HIP(ctx, hipMemcpy(d_bcnt, bcnt.data(), nb * 4, hipMemcpyHostToDevice));
    }
    D2G_HIP(ctx, hipMemset(d_status, 0, 2 * sizeof(int)));
    WsArgs a;
    a.ids = d_ids; a.w = d_w; a.blk_set = d_bset; a.blk_lo = d_blo; a.blk_cnt = d_bcnt;
    a.m = (uint32_t)m; a.h = d_h; a.guess = d_guess; a.redo = d_redo; a.redo_mode = 0; a.status = d_status;
    a.arg = nullptr; a.set_lo = nullptr;
    {
        d2g_timer tm(ctx, &ctx->ev_k3, nullptr);
        const size_t ninit = std::max<size_t>(nsets * m, nsets);
        hipLaunchKernelGGL(k3_bmh_init_kernel, dim3((unsigned)div_up<size_t>(ninit, K3_THREADS)), dim3(K3_THREADS), 0, nullptr,
                           d_h, nsets * m, d_tw, d_redo, nsets);
        D2G_HIP(ctx, hipMemcpy(d_tw, tw.data(), nsets * 8, hipMemcpyHostToDevice));
        if ((rc = ws_walk(ctx, nullptr, a, nsets, nb, d_guess, d_redo, d_tw, d_status))) return rc;
        if (owner_out) {
            if ((rc = d_arg.alloc(ctx, nsets * m, what)) || (rc = d_setlo.alloc(ctx, nsets, what))) return rc;
            D2G_HIP(ctx, hipMemset(d_arg, 0xFF, nsets * m * 8));
            D2G_HIP(ctx, hipMemcpy(d_setlo, set_off, nsets * 8, hipMemcpyHostToDevice));
            a.arg = d_arg; a.set_lo = d_setlo;
            if (nb) hipLaunchKernelGGL(k3_bmh_sets_argmin_kernel, dim3((unsigned)nb), dim3(K3_THREADS), 0, nullptr, a);
        }
        tm.stop();
    }
    D2G_HIP(ctx, hipGetLastError());
    int status = 0;
    D2G_HIP(ctx, hipMemcpy(&status, d_status, sizeof(int), hipMemcpyDeviceToHost));
    D2G_HIP(ctx, hipMemcpy(sig_out, d_h, nsets * m * 8, hipMemcpyDeviceToHost));
    if (owner_out) D2G_HIP(ctx, hipMemcpy(owner_out, d_arg, nsets * m * 8, hipMemcpyDeviceToHost));
    std::memcpy(total_weight_out, tw.data(), nsets * sizeof(double));
    return k3_status_error(ctx, status);
}

}  // extern "C"

// BagMinHash over lists another unit left on the device (K1i's expanded interval runs, d2g_k1i.hip): d2g_bmh_from_weighted_ids without
// the upload of the lists and without the owner pass; the totals and the checks that need them come from the caller's host arrays.
int d2g_bmh_device_lists(d2g_ctx *ctx, hipStream_t s, const uint64_t *ids_dev, const double *w_dev, const uint64_t *set_off, const double *tw,
                         size_t ng, size_t m, double *sig_out, d2g_evlog *ev) {
    D2G_CHECK(ctx, m >= 1 && m < (1ull << 24), "sketchsize out of range");
    D2G_CHECK(ctx, ng < (1ull << 31), "too many sets");
    if (ng == 0) return D2G_OK;
    {   // d2g_bmh_check_weights' last check, on the totals
        const double lnm = std::log((double)m);
        for (size_t i = 0; i < ng; ++i)
            D2G_CHECK(ctx, !(tw[i] > 0.) || ctx->k3_tune.guess_scale * bmh_guess(tw[i], (double)m, lnm) < BMH_GUESS_LIMIT,
                      "BagMinHash: total weight too small for the sketch size (the pruning bound would not stay finite)");
    }
    const std::vector<uint64_t> guess = ws_guesses(tw, ng, m, ctx->k3_tune.guess_scale);
    d2g_ws_blocks wb;
    d2g_ws_plan_blocks(set_off, ng, wb);
    const size_t nb = wb.set.size();
    D2G_CHECK(ctx, nb < (1ull << 31), "too many workgroups");
    d2g_dev<uint64_t> d_blo, d_h, d_guess;
    d2g_dev<double> d_tw;
    d2g_dev<uint32_t> d_bset, d_redo;
    d2g_dev<int> d_status;
    int rc = D2G_OK;
    const char *what = "weighted lists alloc";
    if ((rc = d_blo.alloc(ctx, std::max<size_t>(nb, 1), what)) || (rc = d_bset.alloc(ctx, std::max<size_t>(2 * nb, 1), what)) ||
        (rc = d_h.alloc(ctx, ng * m, what)) || (rc = d_guess.alloc(ctx, ng, what)) || (rc = d_redo.alloc(ctx, ng, what)) ||
        (rc = d_tw.alloc(ctx, ng, what)) || (rc = d_status.alloc(ctx, 2, what))) return rc;
    D2G_HIP(ctx, hipMemcpyAsync(d_guess, guess.data(), ng * 8, hipMemcpyHostToDevice, s));
    if (nb) {
        D2G_HIP(ctx, hipMemcpyAsync(d_blo, wb.lo.data(), nb * 8, hipMemcpyHostToDevice, s));
        D2G_HIP(ctx, hipMemcpyAsync(d_bset, wb.set.data(), nb * 4, hipMemcpyHostToDevice, s));
        D2G_HIP(ctx, hipMemcpyAsync(d_bset + nb, wb.cnt.data(), nb * 4, hipMemcpyHostToDevice, s));
    }
    D2G_HIP(ctx, hipMemsetAsync(d_status, 0, 2 * sizeof(int), s));
    WsArgs a;
    a.ids = ids_dev; a.w = w_dev; a.blk_set = d_bset; a.blk_lo = d_blo; a.blk_cnt = d_bset + nb;
    a.m = (uint32_t)m; a.h = d_h; a.guess = d_guess; a.redo = d_redo; a.redo_mode = 0; a.status = d_status;
    a.arg = nullptr; a.set_lo = nullptr;
    {
        d2g_timer tm(ctx, ev, s);
        const size_t ninit = std::max<size_t>(ng * m, ng);
        hipLaunchKernelGGL(k3_bmh_init_kernel, dim3((unsigned)div_up<size_t>(ninit, K3_THREADS)), dim3(K3_THREADS), 0, s, d_h, ng * m, d_tw, d_redo, ng);
        D2G_HIP(ctx, hipMemcpyAsync(d_tw, tw, ng * 8, hipMemcpyHostToDevice, s));
        rc = ws_walk(ctx, s, a, ng, nb, d_guess, d_redo, d_tw, d_status);
        tm.stop();
    }
    if (rc) { (void)hipStreamSynchronize(s); return rc; }              // the host arrays above are read by copies that may still be in flight
    D2G_HIP(ctx, hipGetLastError());
    int status = 0;
    D2G_HIP(ctx, hipMemcpyAsync(&status, d_status, sizeof(int), hipMemcpyDeviceToHost, s));
    D2G_HIP(ctx, hipMemcpyAsync(sig_out, d_h, ng * m * 8, hipMemcpyDeviceToHost, s));
    D2G_HIP(ctx, hipStreamSynchronize(s));
    return k3_status_error(ctx, status);
}

// =============================================================================================
// K3k: --multiset -c/--countsketch-size/--countmin-size <cells> -- approximate counting in a single-row count-sketch
//   reference src/counter.h:16-19 (the row of `cells` floats), 68-77 (Counter::add(uint64_t)), 131-137 (finalize into the sketch)
// Per k-mer x the walker emits: hv = Wang(maskfn(x)) = Wang(Wang(x ^ XORMASK)), table[hv % cells] += (hv >> 63) ? +1 : -1 -- in int32,
// so the result is the exact integer whatever the order (the reference's float cell stops counting at 2^24: SURVEY F28).  Then every
// cell with |c| >= threshold (and > 0) is one element (id = the cell number, weight = |c|) of BagMinHash.
//   k3k_add      one walk of the k-mers, one atomic add each: into an LDS copy of the genome's row that the workgroup flushes (cells
//                <= L), or straight into the row in global memory
//   k3k_count / k3k_scan / k3k_write   the kept cells of every row, in ascending order, as the (ids, w) lists WsArgs reads
//   k3_bmh_sets / k3_sets_verify (ws_walk)  BagMinHash over those lists where they lie
// A batch whose rows do not fit the table budget goes in groups of consecutive genomes (d2g_cs_groups), each through all three stages.
// =============================================================================================
namespace {

// L: the most cells a workgroup accumulates in LDS.  Measured (profiles/countsketch_time.json, 1000 x 5 Mbp): the LDS form never stops
// winning while the row fits -- its flush is coalesced (consecutive lanes, consecutive cells: full 256-byte atomic wave instructions)
// where the global form issues 64 separate 4-byte requests per wave instruction and runs at about 2.8e10 adds/s for the whole chip.
// 9 ms up to 8192 cells (five workgroups per CU), 11.5 at 16384, 25 at 40960 (one workgroup per CU: the walker loses its occupancy)
// against 136-182 ms in the global form: no crossover below the 160 KiB of LDS, so L is that bound.
constexpr uint32_t K3K_LDS_CELLS = D2G_CS_LDS_MAX;
static_assert(K3K_LDS_CELLS <= D2G_CS_LDS_MAX, "the LDS form holds a whole row");
constexpr int K3K_PER = 16;                              // consecutive cells per lane of the compaction
constexpr int K3K_TILE = K3_THREADS * K3K_PER;           // cells per workgroup of the compaction
constexpr int K3K_SCAN_THREADS = 1024;

struct CsArgs {
    KmerArgs km;
    uint64_t xormask;
    int32_t *table;              // [rows][cells]
    const uint32_t *g_row;       // [n] row of genome g in this group's table
    uint64_t cells;              // 1 .. 2^31
    uint64_t recip;              // floor(2^64 / cells) (not read when cells is a power of two)
};

template <bool FILT, bool WIN, bool AA, bool LDS>
__global__ __launch_bounds__(K1_THREADS) void k3k_add_kernel(CsArgs a) {
    extern __shared__ __attribute__((aligned(16))) int32_t k3k_lds[];
    const uint32_t g = a.km.blk_genome[blockIdx.x + a.km.blk0];
    int32_t *row = a.table + (size_t)a.g_row[g] * a.cells;
    const uint64_t xormask = a.xormask, cells = a.cells, recip = a.recip;
    if constexpr (LDS) {
        const uint32_t C = (uint32_t)cells;
        for (uint32_t i = threadIdx.x; i < C; i += K1_THREADS) k3k_lds[i] = 0;
        __syncthreads();
        d2g_for_each_kmer<FILT, false, WIN, AA>(a.km, [&](uint64_t x) {
            const uint64_t hv = wang64(wang64(x ^ xormask));             // maskfn (src/enums.h:136-140), then counter.h:74
            atomicAdd(&k3k_lds[(uint32_t)d2g_cs_mod(hv, cells, recip)], (hv >> 63) ? 1 : -1);   // BM64 clear: -1 (counter.h:75)
        });
        __syncthreads();
        for (uint32_t i = threadIdx.x; i < C; i += K1_THREADS) {
            const int32_t v = k3k_lds[i];
            if (v) atomicAdd(&row[i], v);                                // the other workgroups of this genome add into the same cells
        }
    } else {
        d2g_for_each_kmer<FILT, false, WIN, AA>(a.km, [&](uint64_t x) {
            const uint64_t hv = wang64(wang64(x ^ xormask));
            atomicAdd(&row[d2g_cs_mod(hv, cells, recip)], (hv >> 63) ? 1 : -1);
        });
    }
}
template <bool LDS> auto k3k_add_fn(bool filt, bool win, bool aa) -> void (*)(CsArgs) {
    return aa ? (filt ? k3k_add_kernel<true, false, true, LDS> : k3k_add_kernel<false, false, true, LDS>)
         : win ? (filt ? k3k_add_kernel<true, true, false, LDS> : k3k_add_kernel<false, true, false, LDS>)
               : (filt ? k3k_add_kernel<true, false, false, LDS> : k3k_add_kernel<false, false, false, LDS>);
}

struct CsListArgs {
    const int32_t *table;        // [rows][cells]
    uint64_t cells;
    uint32_t ntile, rows;        // tiles of K3K_TILE cells per row; workgroup b of count / write owns tile b % ntile of row b / ntile
    double thr;
    uint32_t *tile_cnt;          // [rows * ntile] kept cells
    uint64_t *tile_off;          // [rows * ntile + 1] exclusive prefix: where the tile writes
    uint64_t *row_off;           // [rows + 1] where a row's list begins
    unsigned long long *total;   // [rows] sum of the kept |c|, zeroed by the host
    uint64_t *ids; double *w;    // the lists
};
// the weight a cell passes on: |c| when |c| >= threshold (counter.h:135: >=, not the exact mode's >) and not 0 (BagMinHash2::update
// ignores a weight of 0), else 0.  |c| < 2^31: an input holds fewer k-mers
__device__ __forceinline__ uint32_t k3k_weight(int32_t c, double thr) {
    const uint32_t v = c < 0 ? 0u - (uint32_t)c : (uint32_t)c;
    return (v && (double)v >= thr) ? v : 0u;
}
__global__ __launch_bounds__(K3_THREADS) void k3k_count_kernel(CsListArgs a) {
    __shared__ uint32_t cnt;
    __shared__ unsigned long long ws;
    const uint32_t row = blockIdx.x / a.ntile, t = blockIdx.x % a.ntile;
    if (threadIdx.x == 0) { cnt = 0; ws = 0; }
    __syncthreads();
    const int32_t *tab = a.table + (size_t)row * a.cells;
    const uint64_t c0 = (uint64_t)t * K3K_TILE + (uint64_t)threadIdx.x * K3K_PER;
    uint32_t mine = 0;
    unsigned long long sum = 0;
#pragma unroll
    for (int j = 0; j < K3K_PER; ++j)
        if (c0 + j < a.cells) { const uint32_t v = k3k_weight(tab[c0 + j], a.thr); mine += v != 0; sum += v; }
    if (mine) { atomicAdd(&cnt, mine); atomicAdd(&ws, sum); }
    __syncthreads();
    if (threadIdx.x == 0) { a.tile_cnt[blockIdx.x] = cnt; if (ws) atomicAdd(&a.total[row], ws); }
}
// one workgroup: exclusive prefix over all tiles of the group (row-major: a row's tiles are consecutive, so its list is contiguous and ascending)
__global__ __launch_bounds__(K3K_SCAN_THREADS) void k3k_scan_kernel(CsListArgs a) {
    __shared__ uint64_t part[K3K_SCAN_THREADS];
    const uint32_t tid = threadIdx.x;
    const uint64_t N = (uint64_t)a.rows * a.ntile, per = (N + K3K_SCAN_THREADS - 1) / K3K_SCAN_THREADS;
    const uint64_t lo = tid * per < N ? tid * per : N, hi = lo + per < N ? lo + per : N;
    uint64_t s = 0;
    for (uint64_t i = lo; i < hi; ++i) s += a.tile_cnt[i];
    part[tid] = s;
    __syncthreads();
    for (uint32_t o = 1; o < K3K_SCAN_THREADS; o <<= 1) {
        const uint64_t v = tid >= o ? part[tid - o] : 0;
        __syncthreads();
        part[tid] += v;
        __syncthreads();
    }
    uint64_t run = part[tid] - s;
    for (uint64_t i = lo; i < hi; ++i) {
        a.tile_off[i] = run;
        if (i % a.ntile == 0) a.row_off[i / a.ntile] = run;
        run += a.tile_cnt[i];
    }
    if (tid == K3K_SCAN_THREADS - 1) { a.tile_off[N] = part[tid]; a.row_off[a.rows] = part[tid]; }
}
__global__ __launch_bounds__(K3_THREADS) void k3k_write_kernel(CsListArgs a) {
    __shared__ uint32_t wsum[K3_THREADS / 64];
    if (a.tile_cnt[blockIdx.x] == 0) return;                            // uniform over the workgroup
    const uint32_t tid = threadIdx.x, row = blockIdx.x / a.ntile, t = blockIdx.x % a.ntile;
    const int32_t *tab = a.table + (size_t)row * a.cells;
    const uint64_t c0 = (uint64_t)t * K3K_TILE + (uint64_t)tid * K3K_PER;
    uint32_t v[K3K_PER], mine = 0;
#pragma unroll
    for (int j = 0; j < K3K_PER; ++j) { v[j] = c0 + j < a.cells ? k3k_weight(tab[c0 + j], a.thr) : 0u; mine += v[j] != 0; }
    uint32_t incl = mine;
    for (int o = 1; o < 64; o <<= 1) { const uint32_t u = __shfl_up(incl, o); if ((tid & 63) >= (uint32_t)o) incl += u; }
    if ((tid & 63) == 63) wsum[tid >> 6] = incl;
    __syncthreads();
    uint64_t pos = a.tile_off[blockIdx.x] + (incl - mine);
    for (uint32_t w = 0; w < (tid >> 6); ++w) pos += wsum[w];
#pragma unroll
    for (int j = 0; j < K3K_PER; ++j)
        if (v[j]) { a.ids[pos] = c0 + j; a.w[pos] = (double)v[j]; ++pos; }
}

// what a count-sketch call refuses before it stages or launches anything: the cells, and an input that could overflow an int32 cell
int cs_check(d2g_ctx *ctx, const PackedRuns &in, uint64_t cells) {
    D2G_CHECK(ctx, cells >= 1 && cells <= D2G_CS_MAX_CELLS, "count-sketch: cells must be in [1, 2^31]");
    if (!in.genome_run_off || (in.nrun && !in.run_len) || in.k < 1) return D2G_OK;       // left to the plan's own checks
    for (size_t g = 0; g < in.n; ++g) {
        uint64_t nk = 0;
        for (uint64_t r = in.genome_run_off[g]; r < in.genome_run_off[g + 1] && r < in.nrun; ++r) nk += d2g_run_emissions_of(in.run_len[r], in.k, in.w);
        D2G_CHECK(ctx, nk < D2G_CS_MAX_KMERS, "count-sketch: 2^31 k-mers or more in one input (a cell is an int32)");
    }
    return D2G_OK;
}

// one count-sketch call over a staged batch: what it is to leave behind
struct CsRun {
    uint64_t xormask = 0, cells = 1;
    double thr = 0.;
    int32_t *table_out = nullptr;                                       // host [n][cells]: the signed tables
    bool lists = false;                                                 // host lists: ids_out / w_out [cap], set_off_out [n + 1], total_out [n]
    uint64_t *ids_out = nullptr; double *w_out = nullptr; size_t cap = 0; uint64_t *set_off_out = nullptr, *total_out = nullptr;
    size_t m = 0;                                                       // > 0: BagMinHash registers [n][m] and total weights [n] ...
    double *sig_out = nullptr, *tw_out = nullptr; hipMemcpyKind out = hipMemcpyDeviceToHost;   // ... copied out as `out` says
};

int cs_run(const KmerBatch &b, const CsRun &c) {
    d2g_ctx *ctx = b.ctx;
    K3Run r;
    if (int rc = k3_begin(b, r)) return rc;
    const size_t n = r.n, m = c.m;
    if (n == 0) return D2G_OK;
    d2g_k3_state *st = r.st;
    hipStream_t s = r.s;
    const K3Host &kh = r.kh;
    const uint64_t cells = c.cells;
    D2G_CHECK(ctx, kh.gblk[n] == r.nblk, "internal: K3k block layout disagrees with the launch plan");
    // the table budget: what is free now and what the state already holds; a sixth of it, since a kept cell costs 16 bytes of list
    // beside its 4 of table
    size_t free_b = 0, total_b = 0;
    D2G_HIP(ctx, hipSetDevice(ctx->device));
    D2G_HIP(ctx, hipMemGetInfo(&free_b, &total_b));
    const uint64_t avail = (uint64_t)free_b + st->d_cs_table.cap() * sizeof(int32_t), row_bytes = cells * sizeof(int32_t);
    if (row_bytes > avail) {
        char msg[200];
        std::snprintf(msg, sizeof msg, "count-sketch: one table of %llu cells needs %llu bytes of device memory, %llu are free",
                      (unsigned long long)cells, (unsigned long long)row_bytes, (unsigned long long)avail);
        ctx->last_error = msg;
        return D2G_ERR_NOMEM;
    }
    const uint64_t budget = ctx->k3_tune.cs_table_bytes ? ctx->k3_tune.cs_table_bytes : avail / 6;
    std::vector<uint32_t> row;
    const std::vector<size_t> cut = d2g_cs_groups(kh.gblk.data(), n, cells, budget, row);
    const uint64_t ntile = div_up<uint64_t>(cells, K3K_TILE);
    if (int rc = st->d_cs_row.grow(ctx, n, 4096)) return rc;
    if (!st->d_status) if (int rc = st->d_status.alloc(ctx, 2, "k3 status alloc")) return rc;
    D2G_HIP(ctx, hipMemcpyAsync(st->d_cs_row, row.data(), n * sizeof(uint32_t), hipMemcpyHostToDevice, s));
    D2G_HIP(ctx, hipMemsetAsync(st->d_status, 0, 2 * sizeof(int), s));
    if (m) {
        if (int rc = st->d_h.grow(ctx, std::max<size_t>(n * m, 1), 4096)) return rc;
        if (int rc = st->d_tw.grow(ctx, n, 4096)) return rc;
        if (int rc = st->d_guess.grow(ctx, n, 4096)) return rc;
        if (int rc = st->d_redo.grow(ctx, n, 4096)) return rc;
        r.m = m;
        r.init_registers();
    }
    const int lds_cells = ctx->k3_tune.cs_lds_cells >= 0 ? ctx->k3_tune.cs_lds_cells : (int)K3K_LDS_CELLS;
    const bool lds = cells <= (uint64_t)lds_cells;
    const bool filt = r.km.ftab != nullptr, win = r.km.q > 1, aa = d2g_km_protein(r.km);
    const auto add = lds ? k3k_add_fn<true>(filt, win, aa) : k3k_add_fn<false>(filt, win, aa);
    if (lds) D2G_HIP(ctx, hipFuncSetAttribute((const void *)add, hipFuncAttributeMaxDynamicSharedMemorySize, (int)(cells * sizeof(int32_t))));
    std::vector<uint64_t> rowinfo, set_off, total, guess;
    std::vector<double> tw;
    d2g_ws_blocks wb;
    uint64_t at = 0;                                                    // host lists: elements written so far
    ctx->cs_batches += 1; ctx->cs_groups += cut.size() - 1;
    for (size_t j = 0; j + 1 < cut.size(); ++j) {
        const size_t g0 = cut[j], g1 = cut[j + 1], ng = g1 - g0;
        size_t rows = 0;
        for (size_t g = g0; g < g1; ++g) rows += row[g] != ~0u;
        set_off.assign(ng + 1, 0); total.assign(ng, 0);
        if (rows) {
            // ---- the table: zeroed for exactly rows * cells cells, one walk
            D2G_CHECK(ctx, rows * ntile < (1ull << 31), "count-sketch: too many table tiles in one group; sketch in smaller batches");
            const size_t tcells = rows * cells;
            if (st->d_cs_table.cap() < tcells) if (int rc = st->d_cs_table.alloc(ctx, tcells, "count-sketch table")) return rc;
            ctx->cs_table_bytes = std::max<uint64_t>(ctx->cs_table_bytes, tcells * sizeof(int32_t));
            {
                d2g_timer tm(ctx, &ctx->ev_k3k, s);
                D2G_HIP(ctx, hipMemsetAsync(st->d_cs_table, 0, tcells * sizeof(int32_t), s));
                CsArgs a;
                a.km = r.km; a.km.blk0 = kh.gblk[g0]; a.xormask = c.xormask; a.table = st->d_cs_table; a.g_row = st->d_cs_row;
                a.cells = cells; a.recip = d2g_cs_recip(cells);
                const unsigned nb = kh.gblk[g1] - kh.gblk[g0];
                hipLaunchKernelGGL(add, dim3(nb), dim3(K1_THREADS), lds ? cells * sizeof(int32_t) : 0, s, a);
                tm.stop();
            }
            // ---- the lists: count per tile, prefix, write; only row_off and the totals come back in between
            const size_t N = rows * ntile;
            if (int rc = st->d_cs_tile_cnt.grow(ctx, N, 4096)) return rc;
            if (int rc = st->d_cs_tile_off.grow(ctx, N + 1 + 2 * rows + 1, 4096)) return rc;
            CsListArgs la;
            la.table = st->d_cs_table; la.cells = cells; la.ntile = (uint32_t)ntile; la.rows = (uint32_t)rows; la.thr = c.thr;
            la.tile_cnt = st->d_cs_tile_cnt; la.tile_off = st->d_cs_tile_off; la.row_off = st->d_cs_tile_off + N + 1;
            la.total = reinterpret_cast<unsigned long long *>(la.row_off + rows + 1); la.ids = nullptr; la.w = nullptr;
            rowinfo.assign(2 * rows + 1, 0);
            d2g_timer tm(ctx, &ctx->ev_k3kcompact, s);
            D2G_HIP(ctx, hipMemsetAsync(la.total, 0, rows * sizeof(uint64_t), s));
            hipLaunchKernelGGL(k3k_count_kernel, dim3((unsigned)N), dim3(K3_THREADS), 0, s, la);
            hipLaunchKernelGGL(k3k_scan_kernel, dim3(1), dim3(K3K_SCAN_THREADS), 0, s, la);
            D2G_HIP(ctx, hipMemcpyAsync(rowinfo.data(), la.row_off, rowinfo.size() * sizeof(uint64_t), hipMemcpyDeviceToHost, s));
            D2G_HIP(ctx, hipStreamSynchronize(s));
            const uint64_t nel = rowinfo[rows];
            if (int rc = st->d_cs_ids.grow(ctx, std::max<uint64_t>(nel, 1), 4096)) return rc;
            if (int rc = st->d_cs_w.grow(ctx, std::max<uint64_t>(nel, 1), 4096)) return rc;
            la.ids = st->d_cs_ids; la.w = st->d_cs_w;
            if (nel) hipLaunchKernelGGL(k3k_write_kernel, dim3((unsigned)N), dim3(K3_THREADS), 0, s, la);
            tm.stop();
            d2g_cs_expand_set_off(row.data(), g0, g1, rowinfo.data(), rowinfo.data() + rows + 1, set_off.data(), total.data());
        }
        const uint64_t nel = set_off[ng];
        if (c.table_out) {
            for (size_t g = g0; g < g1; ++g) {
                if (row[g] == ~0u) std::memset(c.table_out + g * cells, 0, cells * sizeof(int32_t));
                else D2G_HIP(ctx, hipMemcpyAsync(c.table_out + g * cells, st->d_cs_table + (size_t)row[g] * cells, cells * sizeof(int32_t), hipMemcpyDeviceToHost, s));
            }
            D2G_HIP(ctx, hipStreamSynchronize(s));
        }
        if (c.lists) {
            D2G_CHECK(ctx, at + nel <= c.cap, "d2g_countsketch_cells: output capacity too small");
            if (nel) {
                D2G_HIP(ctx, hipMemcpyAsync(c.ids_out + at, st->d_cs_ids, nel * sizeof(uint64_t), hipMemcpyDeviceToHost, s));
                D2G_HIP(ctx, hipMemcpyAsync(c.w_out + at, st->d_cs_w, nel * sizeof(double), hipMemcpyDeviceToHost, s));
                D2G_HIP(ctx, hipStreamSynchronize(s));
            }
            for (size_t i = 0; i < ng; ++i) { c.set_off_out[g0 + i] = at + set_off[i]; c.total_out[g0 + i] = total[i]; }
            at += nel;
            c.set_off_out[n] = at;
        }
        if (m && nel) {
            // ---- BagMinHash over the lists where they lie: the workgroup tables and the first guesses are built on the host from
            // set_off and the totals alone (a group without a kept cell keeps its +inf registers and total 0)
            tw.resize(ng);
            for (size_t i = 0; i < ng; ++i) tw[i] = (double)total[i];
            {   // d2g_bmh_check_weights' last check, on the totals (a cell's weight is an integer in [1, 2^31): its first two cannot fail)
                const double lnm = std::log((double)m);
                for (size_t i = 0; i < ng; ++i)
                    D2G_CHECK(ctx, !(tw[i] > 0.) || ctx->k3_tune.guess_scale * bmh_guess(tw[i], (double)m, lnm) < BMH_GUESS_LIMIT,
                              "BagMinHash: total weight too small for the sketch size (the pruning bound would not stay finite)");
            }
            guess = ws_guesses(tw.data(), ng, m, ctx->k3_tune.guess_scale);
            d2g_ws_plan_blocks(set_off.data(), ng, wb);
            const size_t nb = wb.set.size();
            D2G_CHECK(ctx, nb < (1ull << 31), "too many workgroups");
            if (int rc = st->d_cs_blo.grow(ctx, nb, 4096)) return rc;
            if (int rc = st->d_cs_bset.grow(ctx, 2 * nb, 4096)) return rc;
            d2g_timer tm(ctx, &ctx->ev_k3kbmh, s);
            D2G_HIP(ctx, hipMemcpyAsync(st->d_tw + g0, tw.data(), ng * sizeof(double), hipMemcpyHostToDevice, s));
            D2G_HIP(ctx, hipMemcpyAsync(st->d_guess + g0, guess.data(), ng * sizeof(uint64_t), hipMemcpyHostToDevice, s));
            D2G_HIP(ctx, hipMemcpyAsync(st->d_cs_blo, wb.lo.data(), nb * sizeof(uint64_t), hipMemcpyHostToDevice, s));
            D2G_HIP(ctx, hipMemcpyAsync(st->d_cs_bset, wb.set.data(), nb * sizeof(uint32_t), hipMemcpyHostToDevice, s));
            D2G_HIP(ctx, hipMemcpyAsync(st->d_cs_bset + nb, wb.cnt.data(), nb * sizeof(uint32_t), hipMemcpyHostToDevice, s));
            WsArgs a;
            a.ids = st->d_cs_ids; a.w = st->d_cs_w; a.blk_set = st->d_cs_bset; a.blk_lo = st->d_cs_blo; a.blk_cnt = st->d_cs_bset + nb;
            a.m = (uint32_t)m; a.h = st->d_h + g0 * m; a.guess = st->d_guess + g0; a.redo = st->d_redo + g0; a.redo_mode = 0;
            a.status = st->d_status; a.arg = nullptr; a.set_lo = nullptr;
            if (int rc = ws_walk(ctx, s, a, ng, nb, st->d_guess + g0, st->d_redo + g0, st->d_tw + g0, st->d_status)) return rc;
            tm.stop();
            int status = 0;
            D2G_HIP(ctx, hipMemcpyAsync(&status, st->d_status, sizeof(int), hipMemcpyDeviceToHost, s));
            D2G_HIP(ctx, hipStreamSynchronize(s));
            if (int rc = k3_status_error(ctx, status)) return rc;
        }
    }
    D2G_HIP(ctx, hipGetLastError());
    if (m) {
        D2G_HIP(ctx, hipMemcpyAsync(c.sig_out, st->d_h, n * m * sizeof(double), c.out, s));
        D2G_HIP(ctx, hipMemcpyAsync(c.tw_out, st->d_tw, n * sizeof(double), c.out, s));
    }
    D2G_HIP(ctx, hipStreamSynchronize(s));
    return D2G_OK;
}

int cs_sketch_check(d2g_ctx *ctx, const PackedRuns &in, size_t sketchsize, uint64_t cells, double threshold, const double *sig_out, const double *tw_out) {
    if (int rc = bmh_check(ctx, in.n, sketchsize, threshold, sig_out, tw_out)) return rc;
    return cs_check(ctx, in, cells);
}
int sketcher_run_bmh_cs(d2g_sketcher *sk, const PackedRuns &in, uint64_t xormask, size_t sketchsize, uint64_t cells, double threshold,
                        double *sig_out, double *tw_out) {
    if (!sk) return D2G_ERR_INVALID;
    if (int rc = cs_sketch_check(sk->ctx, d2g_sketcher_view(sk, in), sketchsize, cells, threshold, sig_out, tw_out)) return rc;
    KmerBatch b;
    if (int rc = d2g_sketcher_stage(sk, in, &b, nullptr)) return rc;
    CsRun c;
    c.xormask = xormask; c.cells = cells; c.thr = threshold; c.m = sketchsize; c.sig_out = sig_out; c.tw_out = tw_out;
    return cs_run(b, c);
}

}  // namespace

extern "C" {

int d2g_countsketch_lds_cells(void) { return (int)K3K_LDS_CELLS; }

int d2g_countsketch_stats(d2g_ctx *ctx, uint64_t *table_bytes, uint64_t *groups, uint64_t *batches) {
    if (!ctx) return D2G_ERR_INVALID;
    if (table_bytes) *table_bytes = ctx->cs_table_bytes;
    if (groups) *groups = ctx->cs_groups;
    if (batches) *batches = ctx->cs_batches;
    return D2G_OK;
}

int d2g_sketcher_run_bmh_cs(d2g_sketcher *sk, const uint8_t *packed, size_t packed_bytes, const uint64_t *run_start, const uint32_t *run_len,
                            size_t nrun, const uint64_t *genome_run_off, size_t n, int k, int canon, uint64_t xormask, size_t sketchsize,
                            uint64_t cells, double count_threshold, double *sig_out, double *total_weight_out) {
    const PackedRuns in{packed, packed_bytes, run_start, run_len, nrun, genome_run_off, n, k, canon};
    return sketcher_run_bmh_cs(sk, in, xormask, sketchsize, cells, count_threshold, sig_out, total_weight_out);
}

int d2g_bmh_sketch_cs(d2g_ctx *ctx, const uint8_t *packed, size_t packed_bytes, const uint64_t *run_start, const uint32_t *run_len,
                      size_t nrun, const uint64_t *genome_run_off, size_t n, int k, int canon, uint64_t xormask, size_t sketchsize,
                      uint64_t cells, double count_threshold, double *sig_out, double *total_weight_out) {
    const PackedRuns in{packed, packed_bytes, run_start, run_len, nrun, genome_run_off, n, k, canon};
    return d2g_with_sketcher(ctx, [&](d2g_sketcher *sk) {
        return sketcher_run_bmh_cs(sk, in, xormask, sketchsize, cells, count_threshold, sig_out, total_weight_out);
    });
}

int d2g_bmh_sketch_cs_dev(d2g_ctx *ctx, const d2g_oph_plan *plan, const uint8_t *packed_dev, int canon, uint64_t xormask, size_t sketchsize,
                          uint64_t cells, double count_threshold, double *sig_out_dev, double *total_weight_out_dev, void *stream) {
    if (!ctx || !plan) return D2G_ERR_INVALID;
    if (int rc = cs_sketch_check(ctx, plan->runs(canon), sketchsize, cells, count_threshold, sig_out_dev, total_weight_out_dev)) return rc;
    KmerBatch b;
    if (int rc = d2g_plan_batch(ctx, plan, packed_dev, canon, stream, &b)) return rc;
    CsRun c;
    c.xormask = xormask; c.cells = cells; c.thr = count_threshold; c.m = sketchsize; c.sig_out = sig_out_dev; c.tw_out = total_weight_out_dev;
    c.out = hipMemcpyDeviceToDevice;
    return cs_run(b, c);
}

int d2g_countsketch_table(d2g_ctx *ctx, const uint8_t *packed, size_t packed_bytes, const uint64_t *run_start, const uint32_t *run_len,
                          size_t nrun, const uint64_t *genome_run_off, size_t n, int k, int canon, uint64_t xormask, uint64_t cells,
                          int32_t *table_out) {
    const PackedRuns in{packed, packed_bytes, run_start, run_len, nrun, genome_run_off, n, k, canon};
    if (!ctx) return D2G_ERR_INVALID;
    D2G_CHECK(ctx, table_out != nullptr || n == 0, "null output");
    if (int rc = cs_check(ctx, in, cells)) return rc;
    D2G_CHECK(ctx, (uint64_t)n * cells <= (1ull << 28), "d2g_countsketch_table: more than 2^28 cells in all (the dense read-back is for small tables; d2g_countsketch_cells has no such limit)");
    return d2g_with_sketcher(ctx, [&](d2g_sketcher *sk) {
        KmerBatch b;
        if (int rc = d2g_sketcher_stage(sk, in, &b, nullptr)) return rc;
        CsRun c;
        c.xormask = xormask; c.cells = cells; c.thr = 0.; c.table_out = table_out;
        return cs_run(b, c);
    });
}

int d2g_countsketch_cells(d2g_ctx *ctx, const uint8_t *packed, size_t packed_bytes, const uint64_t *run_start, const uint32_t *run_len,
                          size_t nrun, const uint64_t *genome_run_off, size_t n, int k, int canon, uint64_t xormask, uint64_t cells,
                          double count_threshold, uint64_t *ids_out, double *w_out, size_t cap, uint64_t *set_off_out, uint64_t *total_out) {
    const PackedRuns in{packed, packed_bytes, run_start, run_len, nrun, genome_run_off, n, k, canon};
    if (!ctx) return D2G_ERR_INVALID;
    D2G_CHECK(ctx, set_off_out != nullptr && (total_out != nullptr || n == 0), "null output");
    D2G_CHECK(ctx, cap == 0 || (ids_out && w_out), "null output");
    D2G_CHECK(ctx, count_threshold == count_threshold, "count_threshold is NaN");
    if (int rc = cs_check(ctx, in, cells)) return rc;
    for (size_t g = 0; g <= n; ++g) set_off_out[g] = 0;
    return d2g_with_sketcher(ctx, [&](d2g_sketcher *sk) {
        KmerBatch b;
        if (int rc = d2g_sketcher_stage(sk, in, &b, nullptr)) return rc;
        CsRun c;
        c.xormask = xormask; c.cells = cells; c.thr = count_threshold; c.lists = true;
        c.ids_out = ids_out; c.w_out = w_out; c.cap = cap; c.set_off_out = set_off_out; c.total_out = total_out;
        return cs_run(b, c);
    });
}

}  // extern "C"

void d2g_warm_k3() {
    hipFuncAttributes a;
    (void)hipFuncGetAttributes(&a, reinterpret_cast<const void *>(&k3_scan_kernel));     // one code object: the filtered walkers come with it
    d2g_warm_filter();                                                                   // a filtered K3 call counts its survivors first
}
