// d2g_k1i.hip -- K1i: interval sets (BED lines) -> One-Permutation SetSketch registers, and the (id, weight) lists behind --multiset
// (gfx950).  Replaces, per covered position i of a line, the reference chain
//   bed2sketch                    src/bedsketch.cpp:43-55   element = XXH3_64bits(chrom) ^ i
//   OPSetSketch::update           src/oph.h:44-53,176-211   id = Wang(element ^ seed_ ^ 0x533f8c2151b20f97), reg[id mod m] = min(.., id)
//   Counter::add(element, inc)    src/bedsketch.cpp:54      (--multiset) weight += inc, then BagMinHash over (element, weight)
// There is no maskfn in front of the sketch (one Wang hash where K1 has two), no packed stream, no walker: a position costs one XOR,
// one wang64 and the bucket lookup.
//
// Parallel decomposition, K1's (the reference runs one thread per file): a line's positions are cut into chunks of K1_CHUNK = 64
// consecutive positions, one lane owns one chunk at a time; a 256-lane workgroup owns up to K1_BLOCK_CHUNKS = 1024 chunks of ONE file
// and keeps that file's m registers in LDS (ds_min_u64 behind a read-compare filter), then merges them into HBM with
// global_atomic_umin_x2; m beyond 16 384 works against HBM/L2 like K1.  Per chunk a lane reads its line's hash, start and stop (three
// 8-byte words) after a binary search of the workgroup's lines in the chunk prefix.  No scratch, no inter-workgroup communication.
#include "d2g_internal.h"
#include "d2g_intervals.h"
#include "d2g_kmers.h"                // wang64
#include "d2g_countsketch.h"          // d2g_ws_plan_blocks: the workgroup tables of BagMinHash over lists
#include <algorithm>
#include <cmath>
#include <cstring>
#include <new>

// the nine launch tables as 256-byte-aligned pieces of ONE device buffer
struct IntervalLayout {
    size_t hash, start, stop, chunk_off, blk_chunk0, blk_file, blk_nchunks, blk_lo, blk_hi, total;
};

struct d2g_interval_plan {
    d2g_ctx *ctx = nullptr;
    size_t n = 0, nkept = 0, nblk = 0;
    uint64_t npositions = 0;
    std::vector<uint64_t> h_hash, h_start, h_stop, h_file_off;   // the caller's tables, every line: the sweep behind --multiset reads them
    std::vector<uint64_t> file_positions;
    IntervalLayout lay{};
    d2g_dev<uint8_t> d_arena;
    IntervalTables tables() const { return {h_hash.data(), h_start.data(), h_stop.data(), h_hash.size(), h_file_off.data(), n}; }
};

namespace {

struct K1iArgs {
    const uint64_t *iv_hash, *iv_start, *iv_stop;   // [nkept]
    const uint64_t *iv_chunk_off;                   // [nkept + 1]
    const uint64_t *blk_chunk0;
    const uint32_t *blk_file, *blk_nchunks, *blk_lo, *blk_hi;
    uint64_t *regs_out;                             // [n][m], pre-filled with ~0
    uint64_t ophxor;
    uint32_t m;
};

template <bool POW2, bool USE_LDS>
__global__ __launch_bounds__(K1_THREADS) void k1i_oph_kernel(K1iArgs a) {
    extern __shared__ __attribute__((aligned(16))) uint64_t lreg[];
    const int tid = threadIdx.x;
    const uint32_t b = blockIdx.x;
    const uint32_t m = a.m;
    uint64_t *gout = a.regs_out + (size_t)a.blk_file[b] * m;

    if (USE_LDS) {
        for (uint32_t i = tid; i < m; i += K1_THREADS) lreg[i] = ~0ull;
        __syncthreads();
    }
    const uint64_t c0 = a.blk_chunk0[b];
    const uint32_t nc = a.blk_nchunks[b];
    const uint32_t rlo = a.blk_lo[b], rhi = a.blk_hi[b];
    for (int it = 0; it < K1_CPT; ++it) {
        const uint32_t ci_blk = it * K1_THREADS + tid;
        if (ci_blk >= nc) break;
        const uint64_t c = c0 + ci_blk;
        // line containing chunk c (lines of this block only)
        uint32_t lo = rlo, hi = rhi;
        while (hi - lo > 1) {
            const uint32_t mid = (lo + hi) >> 1;
            if (a.iv_chunk_off[mid] <= c) lo = mid; else hi = mid;
        }
        const uint64_t p = a.iv_start[lo] + (c - a.iv_chunk_off[lo]) * K1_CHUNK;   // first position of the chunk
        const uint64_t left = a.iv_stop[lo] - p;
        const int n = left < (uint64_t)K1_CHUNK ? (int)left : K1_CHUNK;
        const uint64_t hx = a.iv_hash[lo] ^ a.ophxor;
#pragma unroll 4
        for (int e = 0; e < n; ++e) {
            const uint64_t id = wang64(hx ^ (p + (uint64_t)e));
            // Schismatic<uint32_t>::mod(size_t): argument narrowed to 32 bits (oph.h:184)
            const uint32_t idx = POW2 ? ((uint32_t)id & (m - 1)) : ((uint32_t)id % m);
            if (USE_LDS) {
                if (id < lreg[idx]) atomicMin((unsigned long long *)&lreg[idx], (unsigned long long)id);
            } else {
                if (id < gout[idx]) atomicMin((unsigned long long *)&gout[idx], (unsigned long long)id);
            }
        }
    }
    if (USE_LDS) {
        __syncthreads();
        for (uint32_t i = tid; i < m; i += K1_THREADS) {
            const uint64_t v = lreg[i];
            if (v != ~0ull) atomicMin((unsigned long long *)&gout[i], (unsigned long long)v);
        }
    }
}

void (*const k1i_kernels[4])(K1iArgs) = {k1i_oph_kernel<false, false>, k1i_oph_kernel<false, true>, k1i_oph_kernel<true, false>,
                                        k1i_oph_kernel<true, true>};

// --multiset: run r covers elements [run_off[r], run_off[r + 1]) of the lists; element e of it is (hash ^ (lo + e), weight)
struct K1iExpandArgs {
    const uint64_t *run_hash, *run_lo, *run_off;    // [nruns], [nruns], [nruns + 1]
    const double *run_w;                            // [nruns]
    uint32_t nruns;
    uint64_t total;
    uint64_t *ids;                                  // [total]
    double *w;                                      // [total]
};
constexpr int K1I_EXPAND_PER_BLOCK = 4096;          // consecutive elements per workgroup: 16 per lane, coalesced 2 KiB stores

__global__ __launch_bounds__(K1_THREADS) void k1i_expand_kernel(K1iExpandArgs a) {
    const uint64_t e0 = (uint64_t)blockIdx.x * K1I_EXPAND_PER_BLOCK;
    for (int it = 0; it < K1I_EXPAND_PER_BLOCK / K1_THREADS; ++it) {
        const uint64_t e = e0 + (uint64_t)it * K1_THREADS + threadIdx.x;
        if (e >= a.total) break;
        uint32_t lo = 0, hi = a.nruns;
        while (hi - lo > 1) {
            const uint32_t mid = (lo + hi) >> 1;
            if (a.run_off[mid] <= e) lo = mid; else hi = mid;
        }
        a.ids[e] = a.run_hash[lo] ^ (a.run_lo[lo] + (e - a.run_off[lo]));
        a.w[e] = a.run_w[lo];
    }
}

IntervalLayout interval_layout(size_t nkept, size_t nblk) {
    IntervalLayout l{};
    size_t off = 0;
    auto piece = [&off](size_t bytes) { const size_t at = off; off = (off + bytes + 255) & ~size_t(255); return at; };
    l.hash = piece(nkept * 8); l.start = piece(nkept * 8); l.stop = piece(nkept * 8); l.chunk_off = piece((nkept + 1) * 8);
    l.blk_chunk0 = piece(nblk * 8);
    l.blk_file = piece(nblk * 4); l.blk_nchunks = piece(nblk * 4); l.blk_lo = piece(nblk * 4); l.blk_hi = piece(nblk * 4);
    l.total = off;
    return l;
}

int check_call(d2g_ctx *ctx, const d2g_interval_plan *plan, size_t sketchsize) {
    D2G_CHECK(ctx, plan->ctx == ctx, "plan belongs to another context");
    D2G_CHECK(ctx, sketchsize >= 1 && sketchsize < (1ull << 31), "sketchsize out of range");
    return D2G_OK;
}

// K1i over a plan: empty registers for its files, then the walk (if there is a block to walk)
int k1i_fill_regs(d2g_ctx *ctx, const d2g_interval_plan *p, size_t m, uint64_t *regs_dev, hipStream_t s) {
    D2G_HIP(ctx, hipSetDevice(ctx->device));
    if (p->n) D2G_HIP(ctx, hipMemsetAsync(regs_dev, 0xFF, p->n * m * sizeof(uint64_t), s));   // registers_ initialise to T(-1): oph.h:147,233
    if (p->nblk == 0) return D2G_OK;
    const uint8_t *ar = p->d_arena;
    auto u64 = [&](size_t at) { return reinterpret_cast<const uint64_t *>(ar + at); };
    auto u32 = [&](size_t at) { return reinterpret_cast<const uint32_t *>(ar + at); };
    const IntervalLayout &l = p->lay;
    const K1iArgs a{u64(l.hash), u64(l.start), u64(l.stop), u64(l.chunk_off), u64(l.blk_chunk0), u32(l.blk_file), u32(l.blk_nchunks),
                    u32(l.blk_lo), u32(l.blk_hi), regs_dev, d2g_oph_xor_const(), (uint32_t)m};
    const bool pow2 = (m & (m - 1)) == 0;
    const size_t lds = m * sizeof(uint64_t);
    const bool use_lds = lds <= 128 * 1024;
    auto kern = k1i_kernels[pow2 * 2 + use_lds];
    if (use_lds && lds > 48 * 1024)
        D2G_HIP(ctx, hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    d2g_timer tm(ctx, &ctx->ev_k1i, s);
    hipLaunchKernelGGL(kern, dim3((unsigned)p->nblk), dim3(K1_THREADS), use_lds ? lds : 0, s, a);
    tm.stop();
    D2G_HIP(ctx, hipGetLastError());
    return D2G_OK;
}

}  // namespace

extern "C" {

void d2g_interval_plan_destroy(d2g_interval_plan *p) {
    if (!p) return;
    (void)hipSetDevice(p->ctx->device);
    delete p;
}

uint64_t d2g_interval_plan_npositions(const d2g_interval_plan *p) { return p ? p->npositions : 0; }

int d2g_interval_plan_create(d2g_ctx *ctx, const uint64_t *chrhash, const uint64_t *start, const uint64_t *stop, size_t nint,
                             const uint64_t *file_off, size_t n, d2g_interval_plan **out) {
    if (!ctx || !out) return D2G_ERR_INVALID;
    *out = nullptr;
    const IntervalTables in{chrhash, start, stop, nint, file_off, n};
    IntervalPlanHost ph;
    std::string err;
    if (int rc = d2g_interval_plan_build(in, ph, err)) { ctx->last_error = err; return rc; }
    D2G_HIP(ctx, hipSetDevice(ctx->device));
    std::unique_ptr<d2g_interval_plan, void (*)(d2g_interval_plan *)> p(new (std::nothrow) d2g_interval_plan(), d2g_interval_plan_destroy);
    if (!p) return D2G_ERR_NOMEM;
    p->ctx = ctx; p->n = n; p->nkept = ph.hash.size(); p->nblk = ph.bf.size(); p->npositions = ph.npositions;
    p->file_positions = ph.file_positions;
    if (nint) { p->h_hash.assign(chrhash, chrhash + nint); p->h_start.assign(start, start + nint); p->h_stop.assign(stop, stop + nint); }
    p->h_file_off.assign(file_off, file_off + n + 1);
    p->lay = interval_layout(p->nkept, p->nblk);
    std::vector<uint8_t> h(p->lay.total);
    auto put = [&h](size_t at, const void *src, size_t bytes) { if (bytes) std::memcpy(h.data() + at, src, bytes); };
    const IntervalLayout &l = p->lay;
    put(l.hash, ph.hash.data(), p->nkept * 8); put(l.start, ph.start.data(), p->nkept * 8); put(l.stop, ph.stop.data(), p->nkept * 8);
    put(l.chunk_off, ph.chunk_off.data(), (p->nkept + 1) * 8);
    put(l.blk_chunk0, ph.bc0.data(), p->nblk * 8);
    put(l.blk_file, ph.bf.data(), p->nblk * 4); put(l.blk_nchunks, ph.bn.data(), p->nblk * 4);
    put(l.blk_lo, ph.blo.data(), p->nblk * 4); put(l.blk_hi, ph.bhi.data(), p->nblk * 4);
    if (int rc = p->d_arena.alloc(ctx, h.size(), "interval plan alloc")) return rc;
    D2G_HIP(ctx, hipMemcpy(p->d_arena, h.data(), h.size(), hipMemcpyHostToDevice));
    *out = p.release();
    return D2G_OK;
}

int d2g_interval_oph_sketch_dev(d2g_ctx *ctx, const d2g_interval_plan *plan, size_t sketchsize, uint64_t *regs_out_dev, void *stream) {
    if (!ctx || !plan) return D2G_ERR_INVALID;
    if (int rc = check_call(ctx, plan, sketchsize)) return rc;
    D2G_CHECK(ctx, regs_out_dev != nullptr || plan->n == 0, "null regs_out");
    return k1i_fill_regs(ctx, plan, d2g_oph_m(sketchsize), regs_out_dev, as_stream(stream));
}

int d2g_interval_oph_sketch(d2g_ctx *ctx, const d2g_interval_plan *plan, size_t sketchsize, uint64_t *regs_out) {
    if (!ctx || !plan) return D2G_ERR_INVALID;
    if (int rc = check_call(ctx, plan, sketchsize)) return rc;
    D2G_CHECK(ctx, regs_out != nullptr || plan->n == 0, "null regs_out");
    if (plan->n == 0) return D2G_OK;
    D2G_HIP(ctx, hipSetDevice(ctx->device));
    const size_t m = d2g_oph_m(sketchsize);
    d2g_dev<uint64_t> d_regs;
    d2g_stream s;
    if (int rc = d_regs.alloc(ctx, plan->n * m, "interval registers alloc")) return rc;
    D2G_HIP(ctx, s.create(hipStreamNonBlocking));
    if (int rc = k1i_fill_regs(ctx, plan, m, d_regs, s)) { (void)hipStreamSynchronize(s); return rc; }
    D2G_HIP(ctx, hipMemcpyAsync(regs_out, d_regs, plan->n * m * sizeof(uint64_t), hipMemcpyDeviceToHost, s));
    D2G_HIP(ctx, hipStreamSynchronize(s));
    return D2G_OK;
}

int d2g_interval_runs(const d2g_interval_plan *plan, int normalize, uint64_t *hash_out, uint64_t *lo_out, uint64_t *hi_out, double *w_out,
                      size_t cap, uint64_t *run_off_out, size_t *nruns) {
    if (!plan || !run_off_out || !nruns || (cap && !(hash_out && lo_out && hi_out && w_out))) return D2G_ERR_INVALID;
    const IntervalTables in = plan->tables();
    std::vector<uint64_t> h, lo, hi;
    std::vector<double> w;
    run_off_out[0] = 0;
    for (size_t f = 0; f < plan->n; ++f) {
        d2g_interval_sweep(in, in.file_off[f], in.file_off[f + 1], normalize != 0, h, lo, hi, w);
        run_off_out[f + 1] = h.size();
    }
    *nruns = h.size();
    const size_t nw = std::min(cap, h.size());
    if (nw) {
        std::memcpy(hash_out, h.data(), nw * 8); std::memcpy(lo_out, lo.data(), nw * 8);
        std::memcpy(hi_out, hi.data(), nw * 8); std::memcpy(w_out, w.data(), nw * 8);
    }
    return D2G_OK;
}

int d2g_interval_bmh_sketch(d2g_ctx *ctx, const d2g_interval_plan *plan, int normalize, size_t sketchsize, double *sig_out,
                            double *total_weight_out) {
    if (!ctx || !plan) return D2G_ERR_INVALID;
    D2G_CHECK(ctx, plan->ctx == ctx, "plan belongs to another context");
    D2G_CHECK(ctx, sketchsize >= 1 && sketchsize < (1ull << 24), "sketchsize out of range");
    const size_t n = plan->n, m = sketchsize;
    D2G_CHECK(ctx, n == 0 || (sig_out && total_weight_out), "null argument");
    if (n == 0) return D2G_OK;
    D2G_HIP(ctx, hipSetDevice(ctx->device));
    const IntervalTables in = plan->tables();
    d2g_stream s;
    D2G_HIP(ctx, s.create(hipStreamNonBlocking));
    d2g_dev<uint64_t> d_ids, d_runs;
    d2g_dev<double> d_w;
    std::vector<uint64_t> h, lo, hi, run_off, set_off, tab;
    std::vector<double> w, tw;
    std::vector<size_t> file_r0;
    for (size_t f0 = 0; f0 < n;) {
        // a group of files: their lists (16 bytes per covered position) in a third of the free device memory (or D2G_INTERVAL_LIST_POSITIONS)
        size_t free_b = 0, total_b = 0;
        D2G_HIP(ctx, hipMemGetInfo(&free_b, &total_b));
        const uint64_t list_positions = ctx->limits.interval_list_positions, budget = list_positions ? list_positions : free_b / 3 / 16;
        h.clear(); lo.clear(); hi.clear(); w.clear();
        set_off.assign(1, 0); tw.clear(); run_off.assign(1, 0); file_r0.clear();
        uint64_t covered = 0;                                                      // of the last file swept
        const size_t f1 = d2g_interval_group(f0, n, budget, [&](size_t f) {
            const size_t r0 = h.size();
            file_r0.push_back(r0);
            d2g_interval_sweep(in, in.file_off[f], in.file_off[f + 1], normalize != 0, h, lo, hi, w);
            covered = 0;
            for (size_t r = r0; r < h.size(); ++r) covered += hi[r] - lo[r];       // <= the file's positions <= 2^44
            return covered;
        });
        if (f1 == f0) {
            char msg[256];
            if (list_positions)
                std::snprintf(msg, sizeof msg, "--multiset interval lists of one file need %llu bytes of device memory (16 per covered position), D2G_INTERVAL_LIST_POSITIONS allows %llu",
                              (unsigned long long)(covered * 16), (unsigned long long)(budget * 16));
            else
                std::snprintf(msg, sizeof msg, "--multiset interval lists of one file need %llu bytes of device memory (16 per covered position), %llu are free",
                              (unsigned long long)(covered * 16), (unsigned long long)free_b);
            ctx->last_error = msg;
            return D2G_ERR_NOMEM;
        }
        const size_t ng = f1 - f0;
        if (file_r0.size() > ng) { const size_t r0 = file_r0[ng]; h.resize(r0); lo.resize(r0); hi.resize(r0); w.resize(r0); }   // the next group takes it
        file_r0.resize(ng);
        file_r0.push_back(h.size());                                               // file g of the group owns runs [file_r0[g], file_r0[g + 1])
        for (size_t g = 0; g < ng; ++g) {
            double t = 0.;
            for (size_t r = file_r0[g]; r < file_r0[g + 1]; ++r) {
                run_off.push_back(run_off.back() + (hi[r] - lo[r]));
                t += w[r] * (double)(hi[r] - lo[r]);
            }
            tw.push_back(t);
            set_off.push_back(run_off.back());
        }
        const size_t nruns = h.size();
        const uint64_t total = set_off.back();
        D2G_CHECK(ctx, nruns < (1ull << 32), "too many runs in one group of files");
        if (total) {
            if (int rc = d_ids.grow(ctx, total, 4096, "interval lists alloc")) return rc;
            if (int rc = d_w.grow(ctx, total, 4096, "interval lists alloc")) return rc;
            // the run tables in one upload: hash, lo, off (nruns + 1), weight bits
            tab.resize(4 * nruns + 1);
            std::memcpy(&tab[0], h.data(), nruns * 8); std::memcpy(&tab[nruns], lo.data(), nruns * 8);
            std::memcpy(&tab[2 * nruns], run_off.data(), (nruns + 1) * 8); std::memcpy(&tab[3 * nruns + 1], w.data(), nruns * 8);
            if (int rc = d_runs.grow(ctx, tab.size(), 4096, "interval runs alloc")) return rc;
            D2G_HIP(ctx, hipMemcpyAsync(d_runs, tab.data(), tab.size() * 8, hipMemcpyHostToDevice, s));
            const K1iExpandArgs a{d_runs, d_runs + nruns, d_runs + 2 * nruns, reinterpret_cast<const double *>(d_runs + 3 * nruns + 1),
                                  (uint32_t)nruns, total, d_ids, d_w};
            const uint64_t nb = div_up<uint64_t>(total, K1I_EXPAND_PER_BLOCK);
            D2G_CHECK(ctx, nb < (1ull << 31), "too many workgroups");
            d2g_timer tm(ctx, &ctx->ev_k1iexpand, s);
            hipLaunchKernelGGL(k1i_expand_kernel, dim3((unsigned)nb), dim3(K1_THREADS), 0, s, a);
            tm.stop();
            D2G_HIP(ctx, hipGetLastError());
        }
        if (int rc = d2g_bmh_device_lists(ctx, s, d_ids, d_w, set_off.data(), tw.data(), ng, m, sig_out + f0 * m, &ctx->ev_k1ibmh)) return rc;
        std::memcpy(total_weight_out + f0, tw.data(), ng * sizeof(double));
        f0 = f1;
    }
    return D2G_OK;
}

}  // extern "C"

void d2g_warm_k1i() {
    hipFuncAttributes a;
    (void)hipFuncGetAttributes(&a, reinterpret_cast<const void *>(&k1i_oph_kernel<true, true>));
}
