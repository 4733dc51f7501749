// d2g_screen.hip -- K1s: `dashing2 contain`, reads screened against a database of sampled k-mers (gfx950).
//
// Replaces the per-k-mer chain of the reference's mash-screen (src/contain_main.cpp:34-59,188-244):
//   kmer2ids.find(maskfn(kmer))  -> ++myres[kmer]                       once per k-mer of every query file
//   for every hit key, for every reference that holds it: ++matches[ref], matchsums[ref] += count
//
//   * The database is nrefs x S masked keys (the <out>.kmer64 of `sketch -s`).  Its DISTINCT keys get dense ids [0, D) in
//     ascending key order (host: sort + unique, O(N S log), d2g_screen_rank_keys in d2g_host.cpp); ref_id[r][j] = the id of key[r][j].
//   * The table is K1f's (d2g_filter.hip): RAW k-mers, raw = WangInverse(key) ^ xormask, linear probing at load <= 0.5, home
//     slot d2g_filter_slot, free slot all ones, the all-ones k-mer behind the slots.  slot_id[slot] is the id of the key there.
//     Keys the walker cannot produce (raw >= 4^k, non-canonical under canon) sit in the table and are never asked for.
//   * screen_count_kernel: the shared walker's hit mode (d2g_kmers.h).  Per k-mer one 8-byte home-slot load, sixteen in flight;
//     a miss ends there (no Wang mix, no LDS); a hit loads its id (4 bytes) and adds 1 to cnt[row][id] with a no-return atomic.
//     Lanes that hit one id are NOT combined first: hits are the rare case of a screen, the adds of a poly-A read serialise in
//     L2 on one word and stay exact.  cnt is additive over calls, so a query can be fed in pieces.
//   * screen_reduce_kernel: one wave per (row, reference) gathers cnt[row][ref_id[r][j]] over j < S: matches = non-zero
//     counters, matchsum = their sum in wrapping u32 -- a key in two registers of r counts twice, as `for refid: kmer2ids[key]` does.
#include "d2g_k1.h"
#include <algorithm>
#include <new>
#include <vector>

struct d2g_screen {
    d2g_ctx *ctx = nullptr;
    int k = 0, canon = 0;
    uint64_t xormask = 0;
    size_t nrefs = 0, S = 0, nrows = 0;
    uint64_t D = 0;                            // distinct keys
    uint64_t slots = 0;                        // a power of two >= 2 D (>= 16)
    std::vector<uint64_t> keys;                // [D] the distinct masked keys, ascending: id -> key
    std::vector<uint64_t> fed;                 // [nrows] k-mers fed to each row since the last reset (the 2^32 guard)
    d2g_dev<uint64_t> d_tab;                   // [slots] raw keys, then [0] != 0: the all-ones k-mer is a key
    d2g_dev<uint32_t> d_slot_id;               // [slots + 1] id of the key in each slot; [slots]: of the all-ones k-mer
    d2g_dev<uint32_t> d_ref_id;                // [nrefs][S]
    d2g_dev<uint32_t> d_cnt;                   // [nrows][D]
    d2g_dev<uint32_t> d_grow;                  // genome -> row of the call in flight (grow-only)
};

namespace {

struct ScreenBuildArgs {
    const uint64_t *raw;           // [D] distinct raw keys, id order
    uint64_t *tab;
    uint32_t *slot_id;
    uint64_t D;
    uint32_t mask, shift;
};

// one thread per distinct key: claim a slot (the keys differ, so a claim is never shared), note the id behind it
__global__ __launch_bounds__(256) void screen_build_kernel(ScreenBuildArgs a) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= a.D) return;
    const uint64_t x = a.raw[i];
    if (x == D2G_FILTER_EMPTY) { a.tab[(size_t)a.mask + 1] = 1; a.slot_id[(size_t)a.mask + 1] = (uint32_t)i; return; }
    uint32_t s = d2g_filter_slot(x, a.shift);
    for (;;) {
        if (a.tab[s] == D2G_FILTER_EMPTY &&
            atomicCAS((unsigned long long *)&a.tab[s], (unsigned long long)D2G_FILTER_EMPTY, (unsigned long long)x) == D2G_FILTER_EMPTY) break;
        s = (s + 1) & a.mask;
    }
    a.slot_id[s] = (uint32_t)i;
}

struct ScreenCountArgs {
    KmerArgs km;                   // km.ftab / fmask / fshift: the screen's table
    const uint32_t *slot_id;
    const uint32_t *genome_row;    // [n] of this launch
    uint32_t *cnt;                 // [nrows][D]
    uint64_t D;
};

template <bool WIN>
__global__ __launch_bounds__(K1_THREADS) void screen_count_kernel(ScreenCountArgs a) {
    uint32_t *const row = a.cnt + (size_t)a.genome_row[a.km.blk_genome[blockIdx.x]] * a.D;
    const uint32_t *const slot_id = a.slot_id;
    d2g_for_each_kmer<true, true, WIN>(a.km, [&](uint64_t, uint32_t slot) {
        (void)atomicAdd(&row[slot_id[slot]], 1u);                // result unused: a non-returning global_atomic_add
    });
}

// wave w of the grid owns pair w = row * nrefs + r of rows [row0, row0 + nrows)
__global__ __launch_bounds__(256) void screen_reduce_kernel(const uint32_t *cnt, const uint32_t *ref_id, uint64_t D, uint32_t S, uint64_t nrefs,
                                                            uint64_t row0, uint64_t npairs, uint32_t *matches, uint32_t *sums) {
    const uint64_t w = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (w >= npairs) return;                                     // a whole wave leaves together
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t row = w / nrefs, r = w - row * nrefs;
    const uint32_t *const c = cnt + (size_t)(row0 + row) * D;
    const uint32_t *const ids = ref_id + (size_t)r * S;
    uint32_t m = 0, sum = 0;
    for (uint32_t j = lane; j < S; j += 64) {
        const uint32_t v = c[ids[j]];
        m += v != 0;
        sum += v;
    }
    for (int o = 32; o; o >>= 1) { m += __shfl_xor(m, o); sum += __shfl_xor(sum, o); }
    if (lane == 0) { matches[w] = m; sums[w] = sum; }
}

int screen_check(d2g_ctx *ctx, const d2g_screen *sc, int k, int canon) {
    D2G_CHECK(ctx, sc->ctx == ctx, "screen belongs to another context");
    D2G_CHECK(ctx, sc->k == k, "screen was built for another k");
    D2G_CHECK(ctx, (sc->canon != 0) == (canon != 0), "screen was built with another canonicalisation");
    return D2G_OK;
}

// the k-mers this call adds to every row, checked against the 2^32 guard; `add` [nrows] comes back filled, nothing is committed.
// Tables that d2g_plan_build will reject (null, not monotone, a run shorter than k) pass: they are left to it.
int screen_account(d2g_ctx *ctx, const d2g_screen *sc, const PackedRuns &in, const uint32_t *genome_row, std::vector<uint64_t> &add) {
    const uint32_t *run_len = in.run_len;
    const uint64_t *genome_run_off = in.genome_run_off;
    const size_t nrun = in.nrun, n = in.n;
    add.assign(sc->nrows, 0);
    D2G_CHECK(ctx, n == 0 || genome_row != nullptr, "null genome_row");
    for (size_t g = 0; g < n; ++g) D2G_CHECK(ctx, genome_row[g] < sc->nrows, "genome_row names a row the screen does not have");
    if (n == 0 || !genome_run_off || (nrun && !run_len)) return D2G_OK;
    for (size_t g = 0; g < n; ++g) {
        if (genome_run_off[g] > genome_run_off[g + 1] || genome_run_off[g + 1] > nrun) return D2G_OK;
        for (uint64_t r = genome_run_off[g]; r < genome_run_off[g + 1]; ++r) {
            if (run_len[r] < (uint32_t)sc->k) return D2G_OK;
            add[genome_row[g]] += d2g_run_emissions_of(run_len[r], sc->k, in.w);
        }
    }
    for (size_t q = 0; q < sc->nrows; ++q)
        if (add[q] && sc->fed[q] + add[q] >= (1ull << 32)) {
            ctx->last_error = "screen row " + std::to_string(q) + " would reach 2^32 k-mers (" + std::to_string(sc->fed[q]) + " fed, " +
                              std::to_string(add[q]) + " more): its uint32 counters could wrap";
            return D2G_ERR_UNSUPPORTED;
        }
    return D2G_OK;
}

// the count walk of one batch on its stream (the table is the screen's: a filter the batch carries plays no part); commits `add`
// once the launch is enqueued
int screen_launch(d2g_screen *sc, const KmerBatch &b, const uint32_t *genome_row, const std::vector<uint64_t> &add) {
    d2g_ctx *ctx = b.ctx;
    hipStream_t s = b.s;
    const size_t nblk = b.nblk, n = b.runs.n;
    KmerArgs km = b.km;
    if (nblk && sc->D) {
        if (int rc = sc->d_grow.grow(ctx, n, 1024, "screen genome rows")) return rc;
        D2G_HIP(ctx, hipMemcpyAsync(sc->d_grow, genome_row, n * sizeof(uint32_t), hipMemcpyHostToDevice, s));
        km.ftab = sc->d_tab.get(); km.fmask = (uint32_t)(sc->slots - 1);
        uint32_t lg = 0; while ((1ull << lg) < sc->slots) ++lg;
        km.fshift = 64 - lg; km.blk0 = 0;
        const ScreenCountArgs a{km, sc->d_slot_id.get(), sc->d_grow.get(), sc->d_cnt.get(), sc->D};
        d2g_timer tm(ctx, &ctx->ev_screen, s);
        hipLaunchKernelGGL(km.q > 1 ? screen_count_kernel<true> : screen_count_kernel<false>, dim3((unsigned)nblk), dim3(K1_THREADS), 0, s, a);
        tm.stop();
        D2G_HIP(ctx, hipGetLastError());
    }
    for (size_t q = 0; q < sc->nrows; ++q) sc->fed[q] += add[q];
    return D2G_OK;
}

}  // namespace

void d2g_warm_screen() {
    hipFuncAttributes a;
    (void)hipFuncGetAttributes(&a, reinterpret_cast<const void *>(&screen_count_kernel<false>));
}

extern "C" {

void d2g_screen_destroy(d2g_screen *sc) {
    if (!sc) return;
    (void)hipSetDevice(sc->ctx->device);
    delete sc;
}

int d2g_screen_create(d2g_ctx *ctx, const uint64_t *keys, size_t nrefs, size_t sketchsize, int k, int canon, uint64_t xormask, size_t nrows,
                      d2g_screen **out) {
    if (!ctx || !out) return D2G_ERR_INVALID;
    *out = nullptr;
    D2G_CHECK(ctx, k >= 1 && k <= 32, "k out of range (1 .. 32)");
    D2G_CHECK(ctx, sketchsize >= 1 && sketchsize < (1ull << 31), "sketchsize out of range");
    D2G_CHECK(ctx, nrows >= 1, "a screen needs at least one query row");
    D2G_CHECK(ctx, nrefs == 0 || keys != nullptr, "null keys");
    // the walker's slot is a uint32 with ~0 = "not in the table" and slots = "the all-ones k-mer" (d2g_filter_find): the table may
    // have at most 2^31 slots, i.e. 2^30 distinct keys (d2g_screen_table_slots).  Refused on the key count, before the ranking.
    if (nrefs > D2G_SCREEN_MAX_KEYS / sketchsize) {
        ctx->last_error = "database of more than 2^30 keys (" + std::to_string(nrefs) + " references x " + std::to_string(sketchsize) +
                          "): its table would pass 2^31 slots, which the probe's 32-bit slot numbers cannot name";
        return D2G_ERR_UNSUPPORTED;
    }
    D2G_HIP(ctx, hipSetDevice(ctx->device));
    d2g_screen *sc = new (std::nothrow) d2g_screen();
    if (!sc) return D2G_ERR_NOMEM;
    std::unique_ptr<d2g_screen, void (*)(d2g_screen *)> owner(sc, d2g_screen_destroy);
    sc->ctx = ctx; sc->k = k; sc->canon = canon != 0; sc->xormask = xormask; sc->nrefs = nrefs; sc->S = sketchsize; sc->nrows = nrows;
    const size_t nkeys = nrefs * sketchsize;
    std::vector<uint32_t> ref_id;
    std::vector<uint64_t> raw;
    d2g_screen_rank_keys(keys, nkeys, xormask, sc->keys, raw, ref_id);    // (d2g_host.cpp: sort + unique, a binary search per position, OpenMP)
    sc->D = sc->keys.size();
    sc->fed.assign(nrows, 0);
    if (int rc = d2g_screen_table_slots(sc->D, &sc->slots)) { ctx->last_error = "screen of more than 2^30 distinct keys"; return rc; }
    // all of it or nothing: the bytes are known before the first allocation
    const size_t cnt_words = std::max<size_t>(nrows * sc->D, 1);
    D2G_CHECK(ctx, sc->D == 0 || nrows <= (~(size_t)0 / 8) / sc->D, "counter matrix too large");
    const size_t need = (sc->slots + 1) * (sizeof(uint64_t) + sizeof(uint32_t)) + std::max<size_t>(nkeys, 1) * sizeof(uint32_t) +
                        cnt_words * sizeof(uint32_t) + std::max<size_t>(sc->D, 1) * sizeof(uint64_t);
    size_t free_b = 0, total_b = 0;
    D2G_HIP(ctx, hipMemGetInfo(&free_b, &total_b));
    if (need > free_b) {
        ctx->last_error = "screen needs " + std::to_string(need) + " bytes of device memory, " + std::to_string(free_b) + " are free";
        return D2G_ERR_NOMEM;
    }
    d2g_dev<uint64_t> d_raw;
    if (int rc = sc->d_tab.alloc(ctx, sc->slots + 1, "screen table")) return rc;
    if (int rc = sc->d_slot_id.alloc(ctx, sc->slots + 1, "screen slot ids")) return rc;
    if (int rc = sc->d_ref_id.alloc(ctx, std::max<size_t>(nkeys, 1), "screen reference ids")) return rc;
    if (int rc = sc->d_cnt.alloc(ctx, cnt_words, "screen counters")) return rc;
    if (int rc = d_raw.alloc(ctx, std::max<size_t>(sc->D, 1), "screen raw keys")) return rc;
    hipStream_t s = nullptr;
    D2G_HIP(ctx, hipMemcpyAsync(d_raw, raw.data(), sc->D * sizeof(uint64_t), hipMemcpyHostToDevice, s));
    D2G_HIP(ctx, hipMemcpyAsync(sc->d_ref_id, ref_id.data(), nkeys * sizeof(uint32_t), hipMemcpyHostToDevice, s));
    D2G_HIP(ctx, hipMemsetAsync(sc->d_cnt, 0, cnt_words * sizeof(uint32_t), s));
    {
        d2g_timer tm(ctx, &ctx->ev_screenbuild, s);
        D2G_HIP(ctx, hipMemsetAsync(sc->d_tab, 0xFF, sc->slots * sizeof(uint64_t), s));
        D2G_HIP(ctx, hipMemsetAsync(sc->d_tab + sc->slots, 0, sizeof(uint64_t), s));
        D2G_HIP(ctx, hipMemsetAsync(sc->d_slot_id, 0, (sc->slots + 1) * sizeof(uint32_t), s));
        if (sc->D) {
            uint32_t lg = 0; while ((1ull << lg) < sc->slots) ++lg;
            const ScreenBuildArgs a{d_raw.get(), sc->d_tab.get(), sc->d_slot_id.get(), sc->D, (uint32_t)(sc->slots - 1), 64 - lg};
            hipLaunchKernelGGL(screen_build_kernel, dim3((unsigned)div_up<uint64_t>(sc->D, 256)), dim3(256), 0, s, a);
        }
        tm.stop();
    }
    D2G_HIP(ctx, hipGetLastError());
    D2G_HIP(ctx, hipStreamSynchronize(s));                          // raw and ref_id leave scope; the table is ready for any stream
    *out = owner.release();
    return D2G_OK;
}

int d2g_screen_reset(d2g_ctx *ctx, d2g_screen *sc) {
    if (!ctx || !sc) return D2G_ERR_INVALID;
    D2G_CHECK(ctx, sc->ctx == ctx, "screen belongs to another context");
    D2G_HIP(ctx, hipSetDevice(ctx->device));
    D2G_HIP(ctx, hipDeviceSynchronize());                           // a count walk may be in flight on any stream
    D2G_HIP(ctx, hipMemset(sc->d_cnt, 0, std::max<size_t>(sc->nrows * sc->D, 1) * sizeof(uint32_t)));
    std::fill(sc->fed.begin(), sc->fed.end(), 0);
    return D2G_OK;
}

int d2g_screen_info(d2g_ctx *ctx, const d2g_screen *sc, uint64_t *ndistinct, size_t *table_bytes, size_t *counter_bytes) {
    if (!ctx || !sc) return D2G_ERR_INVALID;
    D2G_CHECK(ctx, sc->ctx == ctx, "screen belongs to another context");
    if (ndistinct) *ndistinct = sc->D;
    if (table_bytes) *table_bytes = (size_t)(sc->slots + 1) * (sizeof(uint64_t) + sizeof(uint32_t));
    if (counter_bytes) *counter_bytes = sc->nrows * sc->D * sizeof(uint32_t);
    return D2G_OK;
}

int d2g_screen_fed(d2g_ctx *ctx, const d2g_screen *sc, size_t row, uint64_t *nkmers) {
    if (!ctx || !sc || !nkmers) return D2G_ERR_INVALID;
    D2G_CHECK(ctx, sc->ctx == ctx, "screen belongs to another context");
    D2G_CHECK(ctx, row < sc->nrows, "row out of range");
    *nkmers = sc->fed[row];
    return D2G_OK;
}

int d2g_screen_set_fed(d2g_ctx *ctx, d2g_screen *sc, size_t row, uint64_t nkmers) {
    if (!ctx || !sc) return D2G_ERR_INVALID;
    D2G_CHECK(ctx, sc->ctx == ctx, "screen belongs to another context");
    D2G_CHECK(ctx, row < sc->nrows, "row out of range");
    sc->fed[row] = nkmers;
    return D2G_OK;
}

int d2g_screen_add_dev(d2g_ctx *ctx, d2g_screen *sc, const d2g_oph_plan *plan, const uint8_t *packed_dev, const uint32_t *genome_row, void *stream) {
    if (!ctx || !sc || !plan) return D2G_ERR_INVALID;
    if (plan->alphabet != D2G_ALPHABET_DNA) { ctx->last_error = "screen: a k-mer database is DNA; a plan under a protein alphabet cannot be screened"; return D2G_ERR_UNSUPPORTED; }
    const int canon = sc->canon;                                   // a plan carries k, not the canonicalisation: the screen's holds
    if (int rc = screen_check(ctx, sc, plan->k, canon)) return rc;
    std::vector<uint64_t> add;
    if (int rc = screen_account(ctx, sc, plan->runs(canon), genome_row, add)) return rc;
    KmerBatch b;
    if (int rc = d2g_plan_batch(ctx, plan, packed_dev, canon, stream, &b)) return rc;
    return screen_launch(sc, b, genome_row, add);
}

int d2g_sketcher_run_screen(d2g_sketcher *sk, const uint8_t *packed, size_t packed_bytes, const uint64_t *run_start, const uint32_t *run_len,
                            size_t nrun, const uint64_t *genome_run_off, size_t n, int k, int canon, d2g_screen *sc, const uint32_t *genome_row) {
    if (!sk || !sc) return D2G_ERR_INVALID;
    d2g_ctx *ctx = sk->ctx;
    if (sk->alphabet != D2G_ALPHABET_DNA) { ctx->last_error = "screen: a k-mer database is DNA; a sketcher under a protein alphabet cannot screen"; return D2G_ERR_UNSUPPORTED; }
    const PackedRuns in{packed, packed_bytes, run_start, run_len, nrun, genome_run_off, n, k, canon};
    if (int rc = screen_check(ctx, sc, k, canon)) return rc;        // before the stage touches the stream or the buffers
    std::vector<uint64_t> add;
    if (int rc = screen_account(ctx, sc, d2g_sketcher_view(sk, in), genome_row, add)) return rc;
    KmerBatch b;
    if (int rc = d2g_sketcher_stage(sk, in, &b, nullptr)) return rc;
    if (int rc = screen_launch(sc, b, genome_row, add)) return rc;
    D2G_HIP(ctx, hipStreamSynchronize(b.s));
    return D2G_OK;
}

int d2g_screen_result(d2g_ctx *ctx, const d2g_screen *sc, size_t row0, size_t nrows, uint32_t *matches_out, uint32_t *matchsums_out) {
    if (!ctx || !sc) return D2G_ERR_INVALID;
    D2G_CHECK(ctx, sc->ctx == ctx, "screen belongs to another context");
    D2G_CHECK(ctx, row0 <= sc->nrows && nrows <= sc->nrows - row0, "rows out of range");
    const uint64_t npairs = (uint64_t)nrows * sc->nrefs;
    if (npairs == 0) return D2G_OK;
    D2G_CHECK(ctx, matches_out && matchsums_out, "null output");
    D2G_HIP(ctx, hipSetDevice(ctx->device));
    D2G_HIP(ctx, hipDeviceSynchronize());                           // a count walk may be in flight on any stream
    // whole rows per launch, at most 2^30 waves each (SCREEN_RESULT_PAIRS unless D2G_SCREEN_RESULT_PAIRS shrinks it)
    const uint64_t rows_per = std::max<uint64_t>(1, std::min<uint64_t>(nrows, ctx->limits.screen_result_pairs / sc->nrefs));
    d2g_dev<uint32_t> d_res;
    if (int rc = d_res.alloc(ctx, 2 * rows_per * sc->nrefs, "screen result")) return rc;
    for (uint64_t r = 0; r < nrows; r += rows_per) {
        const uint64_t nr = std::min<uint64_t>(rows_per, nrows - r), np = nr * sc->nrefs;
        uint32_t *dm = d_res.get(), *ds = d_res.get() + rows_per * sc->nrefs;
        d2g_timer tm(ctx, &ctx->ev_screenreduce, nullptr);
        hipLaunchKernelGGL(screen_reduce_kernel, dim3((unsigned)div_up<uint64_t>(np, 4)), dim3(256), 0, nullptr, sc->d_cnt.get(), sc->d_ref_id.get(),
                           sc->D, (uint32_t)sc->S, (uint64_t)sc->nrefs, (uint64_t)(row0 + r), np, dm, ds);
        tm.stop();
        D2G_HIP(ctx, hipGetLastError());
        D2G_HIP(ctx, hipMemcpy(matches_out + r * sc->nrefs, dm, np * sizeof(uint32_t), hipMemcpyDeviceToHost));
        D2G_HIP(ctx, hipMemcpy(matchsums_out + r * sc->nrefs, ds, np * sizeof(uint32_t), hipMemcpyDeviceToHost));
    }
    return D2G_OK;
}

int d2g_screen_key_counts(d2g_ctx *ctx, const d2g_screen *sc, size_t row, uint64_t *keys_out, uint32_t *counts_out) {
    if (!ctx || !sc) return D2G_ERR_INVALID;
    D2G_CHECK(ctx, sc->ctx == ctx, "screen belongs to another context");
    D2G_CHECK(ctx, row < sc->nrows, "row out of range");
    if (sc->D == 0) return D2G_OK;
    D2G_HIP(ctx, hipSetDevice(ctx->device));
    D2G_HIP(ctx, hipDeviceSynchronize());
    if (keys_out) std::copy(sc->keys.begin(), sc->keys.end(), keys_out);
    if (counts_out) D2G_HIP(ctx, hipMemcpy(counts_out, sc->d_cnt.get() + row * sc->D, sc->D * sizeof(uint32_t), hipMemcpyDeviceToHost));
    return D2G_OK;
}

}  // extern "C"
