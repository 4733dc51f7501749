// d2g_k3_sets.hip -- K3s: the exact k-mer sets of a batch in sorted form (--set / --countdict, d2g_kmer_sets*), from the (key, count)
// that K3's count leaves per bucket in the counting part of the state (k3_exact_counts, d2g_k3_bmh.hip).
#include "d2g_k3_device.h"
#include <algorithm>

namespace {

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
    if (int rc = st->sets.d_ks_pbits.grow(ctx, n, 4096)) return rc;
    if (int rc = st->sets.d_ks_rbase.grow(ctx, n + 1, 4096)) return rc;
    if (int rc = st->sets.d_ks_cnt.grow(ctx, nranges, 4096)) return rc;
    if (int rc = st->sets.d_ks_off.grow(ctx, nranges + 1, 4096)) return rc;
    if (int rc = st->sets.d_ks_cur.grow(ctx, nranges, 4096)) return rc;
    if (int rc = st->sets.d_ks_setoff.grow(ctx, n + 1, 4096)) return rc;
    if (int rc = st->sets.d_ks_cards.grow(ctx, 2 * n, 4096)) return rc;
    D2G_HIP(ctx, hipMemcpyAsync(st->sets.d_ks_pbits, pbits.data(), n * sizeof(uint32_t), hipMemcpyHostToDevice, s));
    D2G_HIP(ctx, hipMemcpyAsync(st->sets.d_ks_rbase, rbase.data(), (n + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, s));
    D2G_HIP(ctx, hipMemsetAsync(st->sets.d_ks_cnt, 0, nranges * sizeof(uint32_t), s));
    D2G_HIP(ctx, hipMemsetAsync(st->sets.d_ks_cards, 0, 2 * n * sizeof(uint64_t), s));
    KsArgs a{};
    a.src_keys = st->count.d_out_keys; a.src_counts = st->count.d_out_counts; a.bucket_off = st->count.d_bucket_off; a.bucket_nd = st->count.d_bucket_nd;
    a.g_boff = st->count.d_gtab + n; a.n = (uint32_t)n; a.TB = kh.TB; a.g_pbits = st->sets.d_ks_pbits; a.g_rbase = st->sets.d_ks_rbase; a.nranges = nranges;
    a.range_cnt = st->sets.d_ks_cnt; a.range_off = st->sets.d_ks_off; a.cursor = st->sets.d_ks_cur; a.set_off = st->sets.d_ks_setoff; a.cards = st->sets.d_ks_cards;
    a.status = st->count.d_status;
    d2g_timer tm(ctx, &ctx->ev_k3s, s);
    if (kh.TB) hipLaunchKernelGGL(ks_place_kernel<false>, dim3(kh.TB), dim3(K3_THREADS), 0, s, a);
    hipLaunchKernelGGL(ks_scan_kernel, dim3(1), dim3(KS_SCAN_THREADS), 0, s, a);
    uint64_t total = 0;
    D2G_HIP(ctx, hipMemcpyAsync(&total, st->sets.d_ks_off + nranges, sizeof(uint64_t), hipMemcpyDeviceToHost, s));
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
        if (int rc = st->sets.d_ks_counts.grow(ctx, total, 4096)) return rc;
        counts_dev = st->sets.d_ks_counts;
    }
    a.keys = keys_dev; a.counts = counts_dev;
    if (kh.TB && total) {
        hipLaunchKernelGGL(ks_place_kernel<true>, dim3(kh.TB), dim3(K3_THREADS), 0, s, a);
        hipLaunchKernelGGL(ks_sort_kernel, dim3((unsigned)nranges), dim3(K3_THREADS), 0, s, a);
    }
    tm.stop();
    D2G_HIP(ctx, hipGetLastError());
    D2G_HIP(ctx, hipMemcpyAsync(set_off_dev, st->sets.d_ks_setoff, (n + 1) * sizeof(uint64_t), hipMemcpyDeviceToDevice, s));
    D2G_HIP(ctx, hipMemcpyAsync(cards_dev, st->sets.d_ks_cards, 2 * n * sizeof(uint64_t), hipMemcpyDeviceToDevice, s));
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
    if (int rc = st->sets.d_ks_keys.grow(ctx, room, 4096)) return rc;
    if (int rc = st->sets.d_ks_counts.grow(ctx, room, 4096)) return rc;
    d2g_dev<uint64_t> d_meta;                                    // set_off [n+1], cards [n][2]
    if (int rc = d_meta.alloc(ctx, 3 * n + 1, "exact k-mer sets: offsets")) return rc;
    uint64_t total = 0;
    if (int rc = k3_sorted_sets(r, "d2g_kmer_sets", st->sets.d_ks_keys, st->sets.d_ks_counts, std::min<uint64_t>(cap, room), d_meta, d_meta + n + 1, &total))
        return rc;
    if (total) {
        D2G_HIP(ctx, hipMemcpyAsync(keys_out, st->sets.d_ks_keys, total * sizeof(uint64_t), hipMemcpyDeviceToHost, r.s));
        if (counts_out) D2G_HIP(ctx, hipMemcpyAsync(counts_out, st->sets.d_ks_counts, total * sizeof(uint32_t), hipMemcpyDeviceToHost, r.s));
    }
    D2G_HIP(ctx, hipMemcpyAsync(set_off_out, d_meta, (n + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost, r.s));
    D2G_HIP(ctx, hipMemcpyAsync(cards_out, d_meta + n + 1, 2 * n * sizeof(uint64_t), hipMemcpyDeviceToHost, r.s));
    D2G_HIP(ctx, hipStreamSynchronize(r.s));
    return D2G_OK;
}

}  // namespace

extern "C" {

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

}  // extern "C"

void d2g_warm_k3_sets() {
    hipFuncAttributes a;
    (void)hipFuncGetAttributes(&a, reinterpret_cast<const void *>(&ks_scan_kernel));
}
