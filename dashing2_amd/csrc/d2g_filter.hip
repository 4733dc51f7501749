// d2g_filter.hip -- K1f: --filterset, the k-mers of a filter input as a set on the device (gfx950).
//
// Replaces FilterSet in its only reachable form, the sorted hash set (reference src/filterset.h:35-222; built at src/d2.cpp:45-98,
// asked at src/fastxsketch.cpp:385-398 and src/fastxsketchbyseq.cpp:327,370,383,420-423 as `!opts.fs_->in_set(maskfn(x))`).
//
//   * The reference stores maskfn(kmer) = Wang(kmer ^ XORMASK) and looks maskfn(x) up.  maskfn is a bijection, so membership of the
//     masked values IS membership of the raw 2-bit (canonical, when the sketch canonicalises) k-mers.  The table holds RAW k-mers: it
//     does not depend on --seed, and the probe sits in the walker K1, K1b and K3 share (d2g_kmers.h), in front of every hash.
//   * Build: the filter's packed run stream is walked by the launch plan K1 uses; every k-mer claims a slot of an open-addressing
//     table of 64-bit keys with a 64-bit compare-and-swap (global_atomic_cmpswap_x2), linear probing.  The slot count is a power of
//     two >= twice the k-mer OCCURRENCES (>= the distinct k-mers): the load stays <= 0.5 and a probe chain always meets a free slot.
//     Lanes that insert the same key race for the same chain: the loser of a claim sees the winner's key and stops -- each distinct
//     key ends up in the table exactly once, and the claims that succeeded are the distinct count.
//   * Every 64-bit value is a k-mer at k = 32 (A x 32 = 0, forward T x 32 = all ones).  A free slot is all ones; the all-ones k-mer
//     lives in a flag word behind the slots instead, never in a slot.
//   * Probe (d2g_filter_hit): home slot = top bits of kmer * 2^64/phi; the walker issues the home-slot loads of the sixteen k-mers
//     of a packed word together, then answers them in order.  One 8-byte load answers ~70 % of the probes at load 0.5.
#include "d2g_k1.h"
#include <algorithm>
#include <new>
#include <vector>

namespace {

struct FilterBuildArgs {
    KmerArgs km;                   // the filter's own stream and plan (km.ftab unused: the unfiltered walker)
    uint64_t *tab;                 // [slots] keys, [slots] all-ones flag, [slots + 1] distinct keys in the slots
    uint32_t mask, shift;
};

template <bool WIN, bool AA = false>
__global__ __launch_bounds__(K1_THREADS) void filter_build_kernel(FilterBuildArgs a) {
    uint32_t claimed = 0;
    bool ones = false;
    d2g_for_each_kmer<false, false, WIN, AA>(a.km, [&](uint64_t x) {
        if (x == D2G_FILTER_EMPTY) { ones = true; return; }
        uint32_t s = d2g_filter_slot(x, a.shift);
        for (;;) {
            const uint64_t cur = a.tab[s];                       // read first: most occurrences of a filter are repeats or find their slot taken
            if (cur == x) break;
            if (cur == D2G_FILTER_EMPTY) {
                const uint64_t old = atomicCAS((unsigned long long *)&a.tab[s], (unsigned long long)D2G_FILTER_EMPTY, (unsigned long long)x);
                if (old == D2G_FILTER_EMPTY) { ++claimed; break; }
                if (old == x) break;                             // another lane put the same key here first
            }
            s = (s + 1) & a.mask;
        }
    });
    for (int o = 32; o; o >>= 1) claimed += __shfl_xor(claimed, o);
    if ((threadIdx.x & 63) == 0 && claimed) atomicAdd((unsigned long long *)&a.tab[(size_t)a.mask + 2], (unsigned long long)claimed);
    if (ones) a.tab[(size_t)a.mask + 1] = 1;                     // every writer writes the same value
}

// surviving k-mers per genome (K3's layout)
template <bool WIN, bool AA = false>
__global__ __launch_bounds__(K1_THREADS) void filter_survivors_kernel(KmerArgs km, unsigned long long *per_genome) {
    uint32_t c = 0;
    d2g_for_each_kmer<true, false, WIN, AA>(km, [&](uint64_t) { ++c; });
    for (int o = 32; o; o >>= 1) c += __shfl_xor(c, o);
    if ((threadIdx.x & 63) == 0 && c) atomicAdd(&per_genome[km.blk_genome[blockIdx.x]], (unsigned long long)c);
}

// membership of explicit k-mers through the walker's probe
__global__ __launch_bounds__(256) void filter_contains_kernel(KmerArgs km, const uint64_t *kmers, size_t n, uint8_t *out) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const uint64_t x = kmers[i];
    out[i] = d2g_filter_hit(km, x, km.ftab[d2g_filter_slot(x, km.fshift)]) ? 1 : 0;
}

}  // namespace

int d2g_filter_check(d2g_ctx *ctx, const d2g_kmer_filter *f, int k, int canon, int w, int alphabet) {
    if (!f) return D2G_OK;
    D2G_CHECK(ctx, f->ctx == ctx, "k-mer filter belongs to another context");
    D2G_CHECK(ctx, f->alphabet == alphabet, "k-mer filter was built under another alphabet");
    D2G_CHECK(ctx, f->k == k, "k-mer filter was built for another k");
    D2G_CHECK(ctx, (f->canon != 0) == (canon != 0), "k-mer filter was built with another canonicalisation");
    D2G_CHECK(ctx, f->w == d2g_window_norm(k, w), "k-mer filter was built under another window (-w)");
    return D2G_OK;
}

void d2g_filter_args(const d2g_kmer_filter *f, KmerArgs *km) {
    km->ftab = f ? f->d_tab.get() : nullptr;
    km->fmask = f ? (uint32_t)(f->slots - 1) : 0;
    km->fshift = 0;
    if (f) { uint32_t lg = 0; while ((1ull << lg) < f->slots) ++lg; km->fshift = 64 - lg; }
}

int d2g_filter_survivors(d2g_ctx *ctx, const KmerArgs &km, size_t nblk, size_t n, uint64_t *out, hipStream_t s) {
    std::fill(out, out + n, 0);
    if (!nblk || !n) return D2G_OK;
    d2g_dev<unsigned long long> d_cnt;
    if (int rc = d_cnt.alloc(ctx, n, "k-mer filter survivor counts")) return rc;
    D2G_HIP(ctx, hipMemsetAsync(d_cnt, 0, n * sizeof(unsigned long long), s));
    KmerArgs a = km; a.blk0 = 0;
    const auto kern = d2g_walker_variant(km, [](auto, auto w, auto aa) { return filter_survivors_kernel<w(), aa()>; });
    hipLaunchKernelGGL(kern, dim3((unsigned)nblk), dim3(K1_THREADS), 0, s, a, d_cnt.get());
    D2G_HIP(ctx, hipGetLastError());
    D2G_HIP(ctx, hipMemcpyAsync(out, d_cnt, n * sizeof(uint64_t), hipMemcpyDeviceToHost, s));
    D2G_HIP(ctx, hipStreamSynchronize(s));
    return D2G_OK;
}

void d2g_warm_filter() {
    hipFuncAttributes a;
    (void)hipFuncGetAttributes(&a, reinterpret_cast<const void *>(&filter_build_kernel<false>));
}

// the table of the k-mers that the walk of the batch enumerates (nkmers of them), built on its stream; whatever filter the batch
// carries plays no part in building one
static int filter_build(const KmerBatch &b, uint64_t nkmers, d2g_kmer_filter **out) {
    d2g_ctx *ctx = b.ctx;
    hipStream_t s = b.s;
    const int k = b.runs.k, canon = b.runs.canon;
    if (nkmers > (1ull << 31)) {
        ctx->last_error = "k-mer filter of more than 2^31 k-mers (its table would pass 2^32 slots)";
        return D2G_ERR_UNSUPPORTED;
    }
    D2G_HIP(ctx, hipSetDevice(ctx->device));
    d2g_kmer_filter *f = new (std::nothrow) d2g_kmer_filter();
    if (!f) return D2G_ERR_NOMEM;
    std::unique_ptr<d2g_kmer_filter, void (*)(d2g_kmer_filter *)> owner(f, d2g_kmer_filter_destroy);
    f->ctx = ctx; f->k = k; f->canon = canon != 0; f->w = b.runs.w; f->alphabet = b.runs.alphabet; f->noccurrences = nkmers;
    f->slots = 16;
    while (f->slots < 2 * f->noccurrences) f->slots <<= 1;
    if (int rc = f->d_tab.alloc(ctx, f->slots + 2, "k-mer filter table")) return rc;      // out of memory: D2G_ERR_NOMEM, no smaller table
    d2g_timer tm(ctx, &ctx->ev_filter, s);
    D2G_HIP(ctx, hipMemsetAsync(f->d_tab, 0xFF, f->slots * sizeof(uint64_t), s));
    D2G_HIP(ctx, hipMemsetAsync(f->d_tab + f->slots, 0, 2 * sizeof(uint64_t), s));
    if (b.nblk) {
        FilterBuildArgs a;
        KmerArgs self;
        d2g_filter_args(f, &self);
        a.km = b.km;
        a.km.ftab = nullptr;
        a.tab = f->d_tab; a.mask = self.fmask; a.shift = self.fshift;
        const auto kern = d2g_walker_variant(a.km, [](auto, auto w, auto aa) { return filter_build_kernel<w(), aa()>; });
        hipLaunchKernelGGL(kern, dim3((unsigned)b.nblk), dim3(K1_THREADS), 0, s, a);
    }
    tm.stop();
    D2G_HIP(ctx, hipGetLastError());
    *out = owner.release();
    return D2G_OK;
}

extern "C" {

void d2g_kmer_filter_destroy(d2g_kmer_filter *f) {
    if (!f) return;
    (void)hipSetDevice(f->ctx->device);
    delete f;
}

int d2g_kmer_filter_create_dev(d2g_ctx *ctx, const d2g_oph_plan *plan, const uint8_t *packed_dev, int canon, void *stream,
                               d2g_kmer_filter **out) {
    if (!ctx || !plan || !out) return D2G_ERR_INVALID;
    *out = nullptr;
    KmerBatch b;
    if (int rc = d2g_plan_batch(ctx, plan, packed_dev, canon, stream, &b)) return rc;
    return filter_build(b, plan->nkmers, out);
}

int d2g_kmer_filter_create(d2g_ctx *ctx, const uint8_t *packed, size_t packed_bytes, const uint64_t *run_start, const uint32_t *run_len,
                           size_t nrun, int k, int canon, d2g_kmer_filter **out) {
    return d2g_kmer_filter_create_windowed(ctx, packed, packed_bytes, run_start, run_len, nrun, k, canon, 0, out);
}

// the host-pointer forms: a sketcher that lives for the call, under the window or the alphabet asked for
static int filter_create_host(d2g_ctx *ctx, const uint8_t *packed, size_t packed_bytes, const uint64_t *run_start, const uint32_t *run_len,
                              size_t nrun, int k, int canon, int w, int alphabet, d2g_kmer_filter **out) {
    const uint64_t gro[2] = {0, nrun};                            // all runs feed ONE set
    const PackedRuns in{packed, packed_bytes, run_start, run_len, nrun, gro, 1, k, canon};
    if (!ctx || !out) return D2G_ERR_INVALID;
    *out = nullptr;
    return d2g_with_sketcher(ctx, [&](d2g_sketcher *sk) -> int {
        KmerBatch b;
        PlanHost ph;
        if (int rc = d2g_sketcher_set_window(sk, w)) return rc;
        if (int rc = d2g_sketcher_set_alphabet(sk, alphabet)) return rc;
        if (int rc = d2g_sketcher_stage(sk, in, &b, &ph)) return rc;
        d2g_kmer_filter *f = nullptr;
        if (int rc = filter_build(b, ph.nkmers, &f)) return rc;
        const hipError_t e = hipStreamSynchronize(sk->stream);    // the stream and the staged input are released on return
        if (e != hipSuccess) { d2g_kmer_filter_destroy(f); return d2g_hip_status(ctx, e, "k-mer filter build"); }
        *out = f;
        return D2G_OK;
    });
}

int d2g_kmer_filter_create_windowed(d2g_ctx *ctx, const uint8_t *packed, size_t packed_bytes, const uint64_t *run_start,
                                    const uint32_t *run_len, size_t nrun, int k, int canon, int w, d2g_kmer_filter **out) {
    return filter_create_host(ctx, packed, packed_bytes, run_start, run_len, nrun, k, canon, w, D2G_ALPHABET_DNA, out);
}

int d2g_kmer_filter_create_alphabet(d2g_ctx *ctx, const uint8_t *packed, size_t packed_bytes, const uint64_t *run_start,
                                    const uint32_t *run_len, size_t nrun, int k, int alphabet, d2g_kmer_filter **out) {
    return filter_create_host(ctx, packed, packed_bytes, run_start, run_len, nrun, k, 0, 0, alphabet, out);
}

int d2g_kmer_filter_info(d2g_ctx *ctx, const d2g_kmer_filter *f, uint64_t *noccurrences, uint64_t *ndistinct, size_t *table_bytes) {
    if (!ctx || !f) return D2G_ERR_INVALID;
    D2G_CHECK(ctx, f->ctx == ctx, "k-mer filter belongs to another context");
    D2G_HIP(ctx, hipSetDevice(ctx->device));
    uint64_t tail[2] = {0, 0};
    D2G_HIP(ctx, hipDeviceSynchronize());                         // the build may be in flight on any stream
    D2G_HIP(ctx, hipMemcpy(tail, f->d_tab + f->slots, sizeof(tail), hipMemcpyDeviceToHost));
    if (noccurrences) *noccurrences = f->noccurrences;
    if (ndistinct) *ndistinct = tail[1] + (tail[0] != 0);
    if (table_bytes) *table_bytes = (size_t)(f->slots + 2) * sizeof(uint64_t);
    return D2G_OK;
}

int d2g_kmer_filter_contains(d2g_ctx *ctx, const d2g_kmer_filter *f, const uint64_t *kmers, size_t n, uint8_t *out) {
    if (!ctx || !f) return D2G_ERR_INVALID;
    D2G_CHECK(ctx, f->ctx == ctx, "k-mer filter belongs to another context");
    D2G_CHECK(ctx, n == 0 || (kmers && out), "null k-mers or output");
    if (n == 0) return D2G_OK;
    D2G_HIP(ctx, hipSetDevice(ctx->device));
    d2g_dev<uint64_t> d_in;
    d2g_dev<uint8_t> d_out;
    if (int rc = d_in.alloc(ctx, n, "k-mer filter query")) return rc;
    if (int rc = d_out.alloc(ctx, n, "k-mer filter query")) return rc;
    D2G_HIP(ctx, hipDeviceSynchronize());
    D2G_HIP(ctx, hipMemcpy(d_in, kmers, n * sizeof(uint64_t), hipMemcpyHostToDevice));
    KmerArgs km{};
    d2g_filter_args(f, &km);
    hipLaunchKernelGGL(filter_contains_kernel, dim3((unsigned)div_up<size_t>(n, 256)), dim3(256), 0, nullptr, km, d_in.get(), n, d_out.get());
    D2G_HIP(ctx, hipGetLastError());
    D2G_HIP(ctx, hipMemcpy(out, d_out, n, hipMemcpyDeviceToHost));
    return D2G_OK;
}

int d2g_oph_plan_set_filter(d2g_oph_plan *plan, const d2g_kmer_filter *f) {
    if (!plan) return D2G_ERR_INVALID;
    plan->filter = f;
    return D2G_OK;
}

int d2g_sketcher_set_filter(d2g_sketcher *sk, const d2g_kmer_filter *f) {
    if (!sk) return D2G_ERR_INVALID;
    sk->filter = f;
    return D2G_OK;
}

}  // extern "C"
