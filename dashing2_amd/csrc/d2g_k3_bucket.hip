// d2g_k3_bucket.hip -- K3, first half: the bucket layout of a staged batch and the multi-split of its masked k-mer keys into buckets
// (k3_hist / k3_scan / k3_scatter / k3_refine; the compact form k3c_hist / k3c_scan / k3c_scatter).  What the split is for and how
// the buckets are counted: d2g_k3_bmh.hip.  Also where every K3 operation begins (k3_begin) and its work state ends.
#include "d2g_k3_device.h"
#include <algorithm>
#include <new>

namespace {

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
}  // namespace
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

// the tables every mode needs: bucket geometry and key offsets per genome, zeroed bucket counts and status
int K3Run::upload_tables() {
    const uint32_t TB = kh.TB;
    if (int rc = st->count.d_gtab.grow(ctx, 2 * n + 1, 4096)) return rc;
    if (int rc = st->count.d_bucket_cnt.grow(ctx, (size_t)TB + 1, 4096)) return rc;
    if (int rc = st->count.d_bucket_off.grow(ctx, (size_t)TB + 1, 4096)) return rc;
    if (int rc = st->count.d_cursor.grow(ctx, (size_t)TB + 1, 4096)) return rc;
    key_words = kh.compact ? (kh.total + 1) / 2 : kh.total;
    if (int rc = st->count.d_keys.grow(ctx, std::max<uint64_t>(key_words, 1), 4096)) return rc;
    if (!st->count.d_status) if (int rc = st->count.d_status.alloc(ctx, 2, "k3 status alloc")) return rc;
    if (int rc = st->count.d_koff.grow(ctx, n + 1, 4096)) return rc;
    D2G_HIP(ctx, hipMemcpyAsync(st->count.d_gtab, kh.gtab.data(), (2 * n + 1) * sizeof(uint32_t), hipMemcpyHostToDevice, s));
    D2G_HIP(ctx, hipMemcpyAsync(st->count.d_koff, kh.koff.data(), (n + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, s));
    D2G_HIP(ctx, hipMemsetAsync(st->count.d_bucket_cnt, 0, ((size_t)TB + 1) * sizeof(uint32_t), s));
    D2G_HIP(ctx, hipMemsetAsync(st->count.d_status, 0, 2 * sizeof(int), s));
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

// buffers and tables of the bucketing passes
int K3Run::bucket_prepare() {
    d2g_k3_state::Counting &c = st->count;
    if (kh.compact) {
        D2G_CHECK(ctx, kh.gblk[n] == nblk, "internal: K3 block layout disagrees with the launch plan");
        const size_t ntiles = std::max<size_t>(nblk * K1_CPT, 1);
        if (int rc = c.d_gblk.grow(ctx, n + 1, 4096)) return rc;
        if (int rc = c.d_tile_cnt.grow(ctx, ntiles * K3C_MAXB, 4096)) return rc;
        if (int rc = c.d_tile_off.grow(ctx, ntiles * K3C_MAXB, 4096)) return rc;
        D2G_HIP(ctx, hipMemcpyAsync(c.d_gblk, kh.gblk.data(), (n + 1) * sizeof(uint32_t), hipMemcpyHostToDevice, s));
        return D2G_OK;
    }
    if (const size_t nl2 = kh.l2_tb0.size()) {
        // the coarse keys borrow the sub-range buffer: k3_split_kernel (big inputs) runs after the refinement
        if (int rc = c.d_skeys.grow(ctx, std::max<uint64_t>(key_words, 1), 4096)) return rc;
        if (int rc = c.d_l2.grow(ctx, 2 * nl2, 4096)) return rc;
        D2G_HIP(ctx, hipMemcpyAsync(c.d_l2, kh.l2_tb0.data(), nl2 * sizeof(uint32_t), hipMemcpyHostToDevice, s));
        D2G_HIP(ctx, hipMemcpyAsync(c.d_l2 + nl2, kh.l2_bits.data(), nl2 * sizeof(uint32_t), hipMemcpyHostToDevice, s));
    }
    return c.d_blk_coarse.grow(ctx, std::max<size_t>(nblk, 1) << kh.l1bits, 4096);
}

namespace {
// the kernel arguments of a prepared run: the compact / the generic form
K3cArgs k3c_args(const K3Run &r) {
    const d2g_k3_state::Counting &c = r.st->count;
    K3cArgs a{};
    a.km = r.km; a.g_bbits = c.d_gtab; a.g_boff = c.d_gtab + r.n; a.g_koff = c.d_koff; a.g_blk = c.d_gblk;
    a.tile_cnt = c.d_tile_cnt; a.tile_off = c.d_tile_off; a.bucket_cnt = c.d_bucket_cnt; a.bucket_off = c.d_bucket_off;
    a.keys32 = reinterpret_cast<uint32_t *>(c.d_keys.get()); a.hb = r.kh.hb; a.TB = r.kh.TB;
    return a;
}
K3Args k3_args(const K3Run &r) {
    const d2g_k3_state::Counting &c = r.st->count;
    K3Args a{};
    a.km = r.km; a.xormask = r.xormask; a.g_bbits = c.d_gtab; a.g_boff = c.d_gtab + r.n; a.g_koff = c.d_koff;
    a.bucket_cnt = c.d_bucket_cnt; a.bucket_off = c.d_bucket_off; a.cursor = c.d_cursor; a.keys = c.d_keys;
    a.TB = r.kh.TB; a.l1bits = r.kh.l1bits; a.g0 = 0; a.n_genomes = (uint32_t)r.n;
    if (const size_t nl2 = r.kh.l2_tb0.size()) { a.coarse = c.d_skeys; a.l2_tb0 = c.d_l2; a.l2_bits = c.d_l2 + nl2; }
    a.blk_coarse = c.d_blk_coarse;
    return a;
}
}  // namespace

// the keys of genomes [g_lo, g_hi) into their buckets: hist -> scan -> scatter [-> refine].  The compact form (4-byte stored
// words, tile-sorted split: histogram per tile -> per-tile write offsets -> coalesced flush) takes the whole batch only.
int K3Run::bucket(size_t g_lo, size_t g_hi) {
    if (kh.compact) {
        const K3cArgs kc = k3c_args(*this);
        const unsigned nb = (unsigned)nblk;
        const auto hist = d2g_walker_variant(km, [](auto f, auto w, auto aa) { return k3c_hist_kernel<f(), w(), aa()>; });
        if (nb) hipLaunchKernelGGL(hist, dim3(nb), dim3(K1_THREADS), 0, s, kc);
        hipLaunchKernelGGL(k3c_scan_kernel, dim3((unsigned)n), dim3(K3_THREADS), 0, s, kc);
        if (nb) {
            const auto scatter = d2g_walker_variant(km, [](auto f, auto w, auto aa) { return k3c_scatter_kernel<f(), w(), aa()>; });
            D2G_HIP(ctx, hipFuncSetAttribute((const void *)scatter, hipFuncAttributeMaxDynamicSharedMemorySize, (int)sizeof(K3cScatterLds)));
            hipLaunchKernelGGL(scatter, dim3(nb), dim3(K1_THREADS), sizeof(K3cScatterLds), s, kc);
        }
        return D2G_OK;
    }
    K3Args a = k3_args(*this);
    const unsigned blk_lo = kh.gblk[g_lo], nb = (g_lo == 0 && g_hi == n) ? (unsigned)nblk : kh.gblk[g_hi] - blk_lo;
    a.km.blk0 = blk_lo; a.g0 = (uint32_t)g_lo;
    const auto hist = d2g_walker_variant(km, [](auto f, auto w, auto aa) { return k3_hist_kernel<f(), w(), aa()>; });
    const auto scatter = d2g_walker_variant(km, [](auto f, auto w, auto aa) { return k3_scatter_kernel<f(), w(), aa()>; });
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

// what every K3 operation begins with: the work state of the batch's owner (made on first use), the run filled from the batch, the
// bucket layout.  The only place that fills a K3Run's ctx / st / s / n / km / nblk.
int k3_begin(const KmerBatch &b, K3Run &r) {
    if (!*b.k3) *b.k3 = new (std::nothrow) d2g_k3_state();
    if (!*b.k3) return D2G_ERR_NOMEM;
    r.ctx = b.ctx; r.st = *b.k3; r.s = b.s; r.n = b.runs.n; r.km = b.km; r.nblk = b.nblk;
    return k3_layout(b.ctx, b.runs, r.kh);
}

void d2g_k3_state_destroy(d2g_k3_state *st) { delete st; }

void d2g_warm_k3_bucket() {
    hipFuncAttributes a;
    (void)hipFuncGetAttributes(&a, reinterpret_cast<const void *>(&k3_scan_kernel));     // one code object: the filtered walkers come with it
}
