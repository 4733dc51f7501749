// d2g_k1.hip -- K1: 2-bit packed bases -> One-Permutation SetSketch registers (gfx950).
//
// Replaces, per k-mer, the reference chain
//   bns::Encoder::for_each (absent bonsai; call site src/fastxsketch.cpp:416-417)
//   -> maskfn            src/enums.h:136-140      h1 = Wang(kmer ^ XORMASK)
//   -> DHasher/BHasher   src/oph.h:44-53,59       id = Wang(h1 ^ seed_ ^ 0x533f8c2151b20f97)
//   -> update            src/oph.h:176-211        reg[id mod m] = min(reg[..], id)
//
// Parallel decomposition (the reference runs one thread per file, fastxsketch.cpp:302):
//   * a genome's k-mers are cut into chunks of 64 consecutive k-mer start positions; one lane
//     owns one chunk at a time (k-1 base warm-up from a 64-bit window, then 64 rolled steps);
//   * a 256-lane workgroup owns up to 1024 chunks of ONE genome and keeps that genome's m
//     registers in LDS (ds_min_u64 behind a read-compare filter), then merges them into HBM
//     with global_atomic_umin_x2.  min is associative and commutative, so any split is exact.
//   * packed bases are read straight from HBM/L2: lane l reads the 16..20 bytes of its chunk,
//     consecutive lanes read consecutive 16-byte pieces (1 KiB per wave-instruction).
#include "d2g_k1.h"
#include <algorithm>
#include <cstring>
#include <new>
#include <vector>

namespace {

struct K1Args {
    KmerArgs km;
    uint64_t *regs_out;            // [n][m], pre-filled with ~0
    uint64_t xormask;
    uint64_t ophxor;
    uint32_t m;
};

template <bool POW2, bool USE_LDS, bool FILT, bool WIN = false, bool AA = false>
__global__ __launch_bounds__(K1_THREADS) void k1_oph_kernel(K1Args a) {
    extern __shared__ __attribute__((aligned(16))) uint64_t lreg[];
    const int tid = threadIdx.x;
    const uint32_t g = a.km.blk_genome[blockIdx.x];
    const uint32_t m = a.m;
    uint64_t *gout = a.regs_out + (size_t)g * m;

    if (USE_LDS) {
        for (uint32_t i = tid; i < m; i += K1_THREADS) lreg[i] = ~0ull;
        __syncthreads();
    }
    const uint64_t xormask = a.xormask, ophxor = a.ophxor;
    d2g_for_each_kmer<FILT, false, WIN, AA>(a.km, [&](uint64_t x) {
        const uint64_t id = wang64(wang64(x ^ xormask) ^ ophxor);
        // Schismatic<uint32_t>::mod(size_t): argument narrowed to 32 bits (oph.h:184)
        const uint32_t idx = POW2 ? ((uint32_t)id & (m - 1)) : ((uint32_t)id % m);
        if (USE_LDS) {
            if (id < lreg[idx]) atomicMin((unsigned long long *)&lreg[idx], (unsigned long long)id);
        } else {
            if (id < gout[idx]) atomicMin((unsigned long long *)&gout[idx], (unsigned long long)id);
        }
    });
    if (USE_LDS) {
        __syncthreads();
        for (uint32_t i = tid; i < m; i += K1_THREADS) {
            // (a read filter -- skip the atomic when a plain load already shows a value <= v -- was measured: atomic
            // write traffic 0.63 -> 0.12 GB per 1000 genomes, but the 8 KB of register reads per workgroup that replace it
            // and the dependent load at the end of every workgroup made the kernel 1.7 % slower; traffic is not its bound)
            const uint64_t v = lreg[i];
            if (v != ~0ull) atomicMin((unsigned long long *)&gout[i], (unsigned long long)v);
        }
    }
}

// K1b: how often the k-mer behind each FINAL register occurred (LazyOnePermSetSketch::update's counts_, oph.h:207-209, read by
// idcounts(), oph.h:272-277).  A second walk in K1's decomposition, in a launch of its own after K1: a register is final only once
// every workgroup of its genome has merged.  The workgroup keeps its genome's m registers (8 m bytes) and m u32 counters (4 m) in
// LDS: 12 m bytes.  A k-mer counts when its id EQUALS the register it maps to -- an empty register (~0) is compared like any
// other value, so a k-mer whose id is 2^64-1 counts (`cref += (rref == id)`, oph.h:209).
struct K1CountArgs {
    KmerArgs km;
    const uint64_t *regs;          // [n][m], final
    uint32_t *counts_out;          // [n][m], pre-filled with 0
    uint64_t xormask;
    uint64_t ophxor;
    uint32_t m;
};

template <bool POW2, bool USE_LDS, bool FILT, bool WIN = false, bool AA = false>
__global__ __launch_bounds__(K1_THREADS) void k1_oph_count_kernel(K1CountArgs a) {
    extern __shared__ __attribute__((aligned(16))) uint64_t lreg[];
    const int tid = threadIdx.x;
    const uint32_t g = a.km.blk_genome[blockIdx.x];
    const uint32_t m = a.m;
    const uint64_t *greg = a.regs + (size_t)g * m;
    uint32_t *gcnt = a.counts_out + (size_t)g * m;
    uint32_t *lcnt = reinterpret_cast<uint32_t *>(lreg + m);

    if (USE_LDS) {
        for (uint32_t i = tid; i < m; i += K1_THREADS) { lreg[i] = greg[i]; lcnt[i] = 0; }
        __syncthreads();
    }
    const uint64_t xormask = a.xormask, ophxor = a.ophxor;
    d2g_for_each_kmer<FILT, false, WIN, AA>(a.km, [&](uint64_t x) {
        const uint64_t id = wang64(wang64(x ^ xormask) ^ ophxor);
        const uint32_t idx = POW2 ? ((uint32_t)id & (m - 1)) : ((uint32_t)id % m);
        if (USE_LDS) {
            if (lreg[idx] == id) (void)atomicAdd(&lcnt[idx], 1u);     // result unused: a non-returning ds_add_u32
        } else {
            if (greg[idx] == id) (void)atomicAdd(&gcnt[idx], 1u);
        }
    });
    if (USE_LDS) {
        __syncthreads();
        for (uint32_t i = tid; i < m; i += K1_THREADS) {
            const uint32_t c = lcnt[i];
            if (c) (void)atomicAdd(&gcnt[i], c);
        }
    }
}

// the instantiations, indexed by POW2 * 4 + USE_LDS * 2 + FILT; the windowed ones (K1w) behind them, + 8; the amino-acid ones (K1a), + 16
void (*const k1_kernels[24])(K1Args) = {k1_oph_kernel<false, false, false>, k1_oph_kernel<false, false, true>, k1_oph_kernel<false, true, false>,
                                       k1_oph_kernel<false, true, true>,   k1_oph_kernel<true, false, false>, k1_oph_kernel<true, false, true>,
                                       k1_oph_kernel<true, true, false>,   k1_oph_kernel<true, true, true>,
                                       k1_oph_kernel<false, false, false, true>, k1_oph_kernel<false, false, true, true>,
                                       k1_oph_kernel<false, true, false, true>,  k1_oph_kernel<false, true, true, true>,
                                       k1_oph_kernel<true, false, false, true>,  k1_oph_kernel<true, false, true, true>,
                                       k1_oph_kernel<true, true, false, true>,   k1_oph_kernel<true, true, true, true>,
                                       k1_oph_kernel<false, false, false, false, true>, k1_oph_kernel<false, false, true, false, true>,
                                       k1_oph_kernel<false, true, false, false, true>,  k1_oph_kernel<false, true, true, false, true>,
                                       k1_oph_kernel<true, false, false, false, true>,  k1_oph_kernel<true, false, true, false, true>,
                                       k1_oph_kernel<true, true, false, false, true>,   k1_oph_kernel<true, true, true, false, true>};
void (*const k1_count_kernels[24])(K1CountArgs) = {k1_oph_count_kernel<false, false, false>, k1_oph_count_kernel<false, false, true>,
                                                  k1_oph_count_kernel<false, true, false>,  k1_oph_count_kernel<false, true, true>,
                                                  k1_oph_count_kernel<true, false, false>,  k1_oph_count_kernel<true, false, true>,
                                                  k1_oph_count_kernel<true, true, false>,   k1_oph_count_kernel<true, true, true>,
                                                  k1_oph_count_kernel<false, false, false, true>, k1_oph_count_kernel<false, false, true, true>,
                                                  k1_oph_count_kernel<false, true, false, true>,  k1_oph_count_kernel<false, true, true, true>,
                                                  k1_oph_count_kernel<true, false, false, true>,  k1_oph_count_kernel<true, false, true, true>,
                                                  k1_oph_count_kernel<true, true, false, true>,   k1_oph_count_kernel<true, true, true, true>,
                                                  k1_oph_count_kernel<false, false, false, false, true>, k1_oph_count_kernel<false, false, true, false, true>,
                                                  k1_oph_count_kernel<false, true, false, false, true>,  k1_oph_count_kernel<false, true, true, false, true>,
                                                  k1_oph_count_kernel<true, false, false, false, true>,  k1_oph_count_kernel<true, false, true, false, true>,
                                                  k1_oph_count_kernel<true, true, false, false, true>,   k1_oph_count_kernel<true, true, true, false, true>};

// one workgroup per block of the plan; its genome's m registers (K1: 8 bytes each; the count pass: 8 + 4) in LDS while they
// fit the 128 KB asked for at most (m <= 16 384; m <= 10 922), beyond against HBM/L2
template <class Args>
int launch_k1_any(d2g_ctx *ctx, void (*const kerns[24])(Args), const Args &a, size_t nblk, size_t lds_per_reg, d2g_evlog *ev, hipStream_t s) {
    const size_t m = a.m;
    const bool pow2 = (m & (m - 1)) == 0;
    const size_t lds = m * lds_per_reg;
    const bool use_lds = lds <= 128 * 1024;
    auto kern = kerns[(d2g_km_protein(a.km) ? 16 : (a.km.q > 1) * 8) + pow2 * 4 + use_lds * 2 + (a.km.ftab != nullptr)];
    if (use_lds && lds > 48 * 1024)
        D2G_HIP(ctx, hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    d2g_timer tm(ctx, ev, s);
    hipLaunchKernelGGL(kern, dim3((unsigned)nblk), dim3(K1_THREADS), use_lds ? lds : 0, s, a);
    tm.stop();
    D2G_HIP(ctx, hipGetLastError());
    return D2G_OK;
}

// K1 over a batch: empty registers for its genomes, then the walk (if there is a block to walk)
int k1_fill_regs(const KmerBatch &b, size_t m, uint64_t xormask, uint64_t *regs_dev) {
    D2G_HIP(b.ctx, hipMemsetAsync(regs_dev, 0xFF, b.runs.n * m * sizeof(uint64_t), b.s));   // registers_ initialise to T(-1): oph.h:147,233
    if (b.nblk == 0) return D2G_OK;
    const K1Args a{b.km, regs_dev, xormask, d2g_oph_xor_const(), (uint32_t)m};
    return launch_k1_any(b.ctx, k1_kernels, a, b.nblk, sizeof(uint64_t), &b.ctx->ev_k1, b.s);
}

// K1b over the same batch, behind K1 on the same stream: zero counters, then the second walk
int k1_fill_counts(const KmerBatch &b, size_t m, uint64_t xormask, const uint64_t *regs_dev, uint32_t *counts_dev) {
    D2G_HIP(b.ctx, hipMemsetAsync(counts_dev, 0, b.runs.n * m * sizeof(uint32_t), b.s));    // counts_ start at 0: oph.h:148,234
    if (b.nblk == 0) return D2G_OK;
    const K1CountArgs a{b.km, regs_dev, counts_dev, xormask, d2g_oph_xor_const(), (uint32_t)m};
    return launch_k1_any(b.ctx, k1_count_kernels, a, b.nblk, sizeof(uint64_t) + sizeof(uint32_t), &b.ctx->ev_k1count, b.s);
}

// the registers of a batch.  mincount < 2 is the plain sketch, K1 (set_mincount only takes effect above 1: oph.h:154-159); sketch -m c:
// empty registers lowered over the k-mers seen at least `mincount` times (K3o, d2g_k3_bmh.hip), which waits for its status word
int oph_regs(const KmerBatch &b, size_t m, uint64_t xormask, uint32_t mincount, uint64_t *regs_dev) {
    if (mincount < 2) return k1_fill_regs(b, m, xormask, regs_dev);
    D2G_HIP(b.ctx, hipMemsetAsync(regs_dev, 0xFF, b.runs.n * m * sizeof(uint64_t), b.s));
    return b.nblk ? d2g_k3_ophmin(b, xormask, m, mincount, regs_dev) : D2G_OK;
}

// what every K1 form refuses alike
int check_sketchsize(d2g_ctx *ctx, size_t sketchsize) {
    D2G_CHECK(ctx, sketchsize >= 1 && sketchsize < (1ull << 31), "sketchsize out of range");
    return D2G_OK;
}

// the sketcher forms: the batch staged on the sketcher's stream, the registers (and, `counts`, K1b over them: LazyOnePermSetSketch's
// counts_ under set_mincount, oph.h:188-205, is what K1b defines for any registers) behind it, the results copied back, ONE wait
int sketcher_run(d2g_sketcher *sk, const PackedRuns &in, uint64_t xormask, size_t sketchsize, uint32_t mincount, uint64_t *regs_out,
                 uint32_t *counts_out, bool counts) {
    if (!sk) return D2G_ERR_INVALID;
    d2g_ctx *ctx = sk->ctx;
    const size_t n = in.n;
    if (int rc = check_sketchsize(ctx, sketchsize)) return rc;
    D2G_CHECK(ctx, (regs_out != nullptr && (counts_out != nullptr || !counts)) || n == 0, counts ? "null regs_out or counts_out" : "null regs_out");
    if (counts) {                                                                     // before the stage touches the device stream
        std::string err;
        if (int rc = d2g_plan_err(ctx, d2g_plan_check_count_range(d2g_sketcher_view(sk, in), err), err)) return rc;
    }
    KmerBatch b;
    if (int rc = d2g_sketcher_stage(sk, in, &b, nullptr)) return rc;
    const size_t m = d2g_oph_m(sketchsize), nm = std::max<size_t>(n * m, 1);
    if (int rc = sk->d_regs.grow(ctx, nm, 4096)) return rc;
    if (counts) if (int rc = sk->d_counts.grow(ctx, nm, 4096)) return rc;
    if (int rc = oph_regs(b, m, xormask, mincount, sk->d_regs)) return rc;
    if (counts) if (int rc = k1_fill_counts(b, m, xormask, sk->d_regs, sk->d_counts)) return rc;
    if (n) D2G_HIP(ctx, hipMemcpyAsync(regs_out, sk->d_regs, n * m * sizeof(uint64_t), hipMemcpyDeviceToHost, b.s));
    if (n && counts) D2G_HIP(ctx, hipMemcpyAsync(counts_out, sk->d_counts, n * m * sizeof(uint32_t), hipMemcpyDeviceToHost, b.s));
    D2G_HIP(ctx, hipStreamSynchronize(b.s));
    return D2G_OK;
}

}  // namespace

extern "C" {

void d2g_oph_plan_destroy(d2g_oph_plan *p) {
    if (!p) return;
    (void)hipSetDevice(p->ctx->device);
    delete p;
}

uint64_t d2g_oph_plan_nkmers(const d2g_oph_plan *p) { return p ? p->nkmers : 0; }
uint64_t d2g_oph_plan_nbases(const d2g_oph_plan *p) { return p ? p->nbases : 0; }

int d2g_oph_plan_create(d2g_ctx *ctx, const uint64_t *run_start, const uint32_t *run_len, size_t nrun,
                        const uint64_t *genome_run_off, size_t n, int k, d2g_oph_plan **out) {
    return d2g_oph_plan_create_windowed(ctx, run_start, run_len, nrun, genome_run_off, n, k, 0, out);
}

namespace {
int oph_plan_create(d2g_ctx *ctx, const PackedRuns &in, d2g_oph_plan **out);
}

int d2g_oph_plan_create_windowed(d2g_ctx *ctx, const uint64_t *run_start, const uint32_t *run_len, size_t nrun,
                                 const uint64_t *genome_run_off, size_t n, int k, int w, d2g_oph_plan **out) {
    const PackedRuns in{nullptr, 0, run_start, run_len, nrun, genome_run_off, n, k, 0, d2g_window_norm(k, w)};   // a plan is made without a stream
    return oph_plan_create(ctx, in, out);
}

int d2g_oph_plan_create_alphabet(d2g_ctx *ctx, const uint64_t *run_start, const uint32_t *run_len, size_t nrun,
                                 const uint64_t *genome_run_off, size_t n, int k, int alphabet, d2g_oph_plan **out) {
    const PackedRuns in{nullptr, 0, run_start, run_len, nrun, genome_run_off, n, k, 0, 0, alphabet};
    return oph_plan_create(ctx, in, out);
}

}  // extern "C"

namespace {
int oph_plan_create(d2g_ctx *ctx, const PackedRuns &in, d2g_oph_plan **out) {
    const size_t nrun = in.nrun, n = in.n;
    if (!ctx || !out) return D2G_ERR_INVALID;
    *out = nullptr;
    PlanHost ph;
    std::string err;
    if (int rc = d2g_plan_err(ctx, d2g_plan_build(in, ph, err), err)) return rc;
    D2G_HIP(ctx, hipSetDevice(ctx->device));
    std::unique_ptr<d2g_oph_plan, void (*)(d2g_oph_plan *)> p(new (std::nothrow) d2g_oph_plan(), d2g_oph_plan_destroy);
    if (!p) return D2G_ERR_NOMEM;
    p->ctx = ctx; p->k = in.k; p->w = in.w; p->alphabet = in.alphabet; p->n = n; p->nrun = nrun;
    p->h_run_len.assign(in.run_len, in.run_len + nrun);
    p->h_genome_run_off.assign(in.genome_run_off, in.genome_run_off + n + 1);
    p->nkmers = ph.nkmers; p->nbases = ph.nbases; p->nblk = ph.bg.size();
    p->lay = d2g_plan_layout(nrun, p->nblk);
    std::vector<uint8_t> h(p->lay.total);
    d2g_plan_fill(h.data(), p->lay, in, ph);
    if (int rc = p->d_arena.alloc(ctx, h.size(), "oph plan alloc")) return rc;
    D2G_HIP(ctx, hipMemcpy(p->d_arena, h.data(), h.size(), hipMemcpyHostToDevice));
    *out = p.release();
    return D2G_OK;
}
}  // namespace

extern "C" {

int d2g_oph_sketch_dev(d2g_ctx *ctx, const d2g_oph_plan *plan, const uint8_t *packed_dev, int canon,
                       uint64_t xormask, size_t sketchsize, uint64_t *regs_out_dev, void *stream) {
    if (!ctx || !plan) return D2G_ERR_INVALID;
    if (int rc = check_sketchsize(ctx, sketchsize)) return rc;
    D2G_CHECK(ctx, regs_out_dev != nullptr, "null regs_out");
    KmerBatch b;
    if (int rc = d2g_plan_batch(ctx, plan, packed_dev, canon, stream, &b)) return rc;
    return k1_fill_regs(b, d2g_oph_m(sketchsize), xormask, regs_out_dev);
}

int d2g_oph_count_dev(d2g_ctx *ctx, const d2g_oph_plan *plan, const uint8_t *packed_dev, int canon, uint64_t xormask,
                      size_t sketchsize, const uint64_t *regs_dev, uint32_t *counts_out_dev, void *stream) {
    if (!ctx || !plan) return D2G_ERR_INVALID;
    if (int rc = check_sketchsize(ctx, sketchsize)) return rc;
    D2G_CHECK(ctx, regs_dev != nullptr && counts_out_dev != nullptr, "null regs or counts_out");
    KmerBatch b;
    if (int rc = d2g_plan_batch(ctx, plan, packed_dev, canon, stream, &b)) return rc;
    return k1_fill_counts(b, d2g_oph_m(sketchsize), xormask, regs_dev, counts_out_dev);
}

int d2g_oph_sketch_mincount_dev(d2g_ctx *ctx, const d2g_oph_plan *plan, const uint8_t *packed_dev, int canon, uint64_t xormask,
                                size_t sketchsize, uint32_t mincount, uint64_t *regs_out_dev, void *stream) {
    if (!ctx || !plan) return D2G_ERR_INVALID;
    if (int rc = check_sketchsize(ctx, sketchsize)) return rc;
    D2G_CHECK(ctx, regs_out_dev != nullptr || plan->n == 0, "null regs_out");
    KmerBatch b;
    if (int rc = d2g_plan_batch(ctx, plan, packed_dev, canon, stream, &b)) return rc;
    if (int rc = oph_regs(b, d2g_oph_m(sketchsize), xormask, mincount, regs_out_dev)) return rc;
    D2G_HIP(ctx, hipStreamSynchronize(b.s));
    return D2G_OK;
}

void d2g_sketcher_destroy(d2g_sketcher *sk) {
    if (!sk) return;
    (void)hipSetDevice(sk->ctx->device);
    (void)hipStreamSynchronize(sk->stream);      // a call that failed behind its stage may have left copies from the pinned buffers in flight
    if (sk->k3) d2g_k3_state_destroy(sk->k3);
    if (sk->k0) d2g_k0_state_destroy(sk->k0);
    delete sk;
}

int d2g_sketcher_create(d2g_ctx *ctx, d2g_sketcher **out) {
    if (!ctx || !out) return D2G_ERR_INVALID;
    *out = nullptr;
    D2G_HIP(ctx, hipSetDevice(ctx->device));
    d2g_sketcher *sk = new (std::nothrow) d2g_sketcher();
    if (!sk) return D2G_ERR_NOMEM;
    sk->ctx = ctx;
    hipError_t e = sk->stream.create(hipStreamNonBlocking);
    if (e != hipSuccess) { ctx->last_error = hipGetErrorString(e); delete sk; return D2G_ERR_HIP; }
    *out = sk;
    return D2G_OK;
}

int d2g_sketcher_set_window(d2g_sketcher *sk, int w) {
    if (!sk) return D2G_ERR_INVALID;
    sk->w = w > 0 ? w : 0;                       // compared with k by every run: w <= k is no window
    return D2G_OK;
}

int d2g_sketcher_set_alphabet(d2g_sketcher *sk, int alphabet) {
    if (!sk) return D2G_ERR_INVALID;
    D2G_CHECK(sk->ctx, alphabet == D2G_ALPHABET_DNA || d2g_alphabet_size(alphabet) > 0, "unknown alphabet");
    sk->alphabet = alphabet;
    return D2G_OK;
}

int d2g_sketcher_run(d2g_sketcher *sk, const uint8_t *packed, size_t packed_bytes, const uint64_t *run_start,
                     const uint32_t *run_len, size_t nrun, const uint64_t *genome_run_off, size_t n, int k, int canon,
                     uint64_t xormask, size_t sketchsize, uint64_t *regs_out) {
    const PackedRuns in{packed, packed_bytes, run_start, run_len, nrun, genome_run_off, n, k, canon};
    return sketcher_run(sk, in, xormask, sketchsize, 0, regs_out, nullptr, false);
}

int d2g_sketcher_run_counts(d2g_sketcher *sk, const uint8_t *packed, size_t packed_bytes, const uint64_t *run_start,
                            const uint32_t *run_len, size_t nrun, const uint64_t *genome_run_off, size_t n, int k, int canon,
                            uint64_t xormask, size_t sketchsize, uint64_t *regs_out, uint32_t *counts_out) {
    const PackedRuns in{packed, packed_bytes, run_start, run_len, nrun, genome_run_off, n, k, canon};
    return sketcher_run(sk, in, xormask, sketchsize, 0, regs_out, counts_out, true);
}

int d2g_oph_sketch(d2g_ctx *ctx, const uint8_t *packed, size_t packed_bytes, const uint64_t *run_start,
                   const uint32_t *run_len, size_t nrun, const uint64_t *genome_run_off, size_t n, int k,
                   int canon, uint64_t xormask, size_t sketchsize, uint64_t *regs_out) {
    const PackedRuns in{packed, packed_bytes, run_start, run_len, nrun, genome_run_off, n, k, canon};
    return d2g_with_sketcher(ctx, [&](d2g_sketcher *sk) { return sketcher_run(sk, in, xormask, sketchsize, 0, regs_out, nullptr, false); });
}

int d2g_oph_sketch_counts(d2g_ctx *ctx, const uint8_t *packed, size_t packed_bytes, const uint64_t *run_start,
                          const uint32_t *run_len, size_t nrun, const uint64_t *genome_run_off, size_t n, int k,
                          int canon, uint64_t xormask, size_t sketchsize, uint64_t *regs_out, uint32_t *counts_out) {
    const PackedRuns in{packed, packed_bytes, run_start, run_len, nrun, genome_run_off, n, k, canon};
    return d2g_with_sketcher(ctx, [&](d2g_sketcher *sk) { return sketcher_run(sk, in, xormask, sketchsize, 0, regs_out, counts_out, true); });
}

int d2g_sketcher_run_mincount(d2g_sketcher *sk, const uint8_t *packed, size_t packed_bytes, const uint64_t *run_start,
                              const uint32_t *run_len, size_t nrun, const uint64_t *genome_run_off, size_t n, int k, int canon,
                              uint64_t xormask, size_t sketchsize, uint32_t mincount, uint64_t *regs_out, uint32_t *counts_out) {
    const PackedRuns in{packed, packed_bytes, run_start, run_len, nrun, genome_run_off, n, k, canon};
    return sketcher_run(sk, in, xormask, sketchsize, mincount, regs_out, counts_out, counts_out != nullptr);
}

int d2g_oph_sketch_mincount(d2g_ctx *ctx, const uint8_t *packed, size_t packed_bytes, const uint64_t *run_start,
                            const uint32_t *run_len, size_t nrun, const uint64_t *genome_run_off, size_t n, int k, int canon,
                            uint64_t xormask, size_t sketchsize, uint32_t mincount, uint64_t *regs_out, uint32_t *counts_out) {
    const PackedRuns in{packed, packed_bytes, run_start, run_len, nrun, genome_run_off, n, k, canon};
    return d2g_with_sketcher(ctx, [&](d2g_sketcher *sk) {
        return sketcher_run(sk, in, xormask, sketchsize, mincount, regs_out, counts_out, counts_out != nullptr);
    });
}

}  // extern "C"

int d2g_plan_batch(d2g_ctx *ctx, const d2g_oph_plan *plan, const uint8_t *packed_dev, int canon, void *stream, KmerBatch *out) {
    D2G_CHECK(ctx, plan->ctx == ctx, "plan belongs to another context");
    D2G_CHECK(ctx, ((uintptr_t)packed_dev & 3) == 0, "packed stream must be 4-byte aligned");
    D2G_CHECK(ctx, plan->nblk == 0 || packed_dev != nullptr, "null packed stream");
    D2G_CHECK(ctx, plan->alphabet == D2G_ALPHABET_DNA || canon == 0, "a protein alphabet has no canonical k-mers: canon must be 0");
    if (int rc = d2g_filter_check(ctx, plan->filter, plan->k, canon, plan->w, plan->alphabet)) return rc;
    D2G_HIP(ctx, hipSetDevice(ctx->device));
    *out = KmerBatch{ctx, as_stream(stream), d2g_plan_kmer_args(plan->d_arena, plan->lay, packed_dev, plan->k, canon, plan->w, plan->alphabet), plan->nblk, plan->runs(canon),
                     &ctx->k3};
    d2g_filter_args(plan->filter, &out->km);
    return D2G_OK;
}

int d2g_sketcher_stage(d2g_sketcher *sk, const PackedRuns &caller, KmerBatch *out, PlanHost *ph_out) {
    d2g_ctx *ctx = sk->ctx;
    PackedRuns in = d2g_sketcher_view(sk, caller);
    if (int rc = d2g_filter_check(ctx, sk->filter, in.k, in.canon, in.w, in.alphabet)) return rc;   // before the stream, the buffers or an output are touched
    uint64_t ingested_bases = 0;
    const bool use_ingested = in.packed == nullptr && d2g_k0_ingested(sk, &ingested_bases);
    D2G_CHECK(ctx, !(use_ingested && in.alphabet != D2G_ALPHABET_DNA), "the ingested stream is DNA: a protein alphabet needs a packed stream");
    D2G_CHECK(ctx, in.nrun == 0 || (in.run_start && (in.packed || use_ingested)), "null input");   // refused with an ingested stream left usable
    if (use_ingested) in.packed_bytes = (size_t)((ingested_bases + 3) / 4 + 64);      // the device stream's extent (zero-padded by the ingest)
    else d2g_k0_invalidate(sk);                                                       // the device buffer is about to be overwritten
    PlanHost ph_local;
    PlanHost &ph = ph_out ? *ph_out : ph_local;
    std::string err;
    if (int rc = d2g_plan_err(ctx, d2g_plan_build(in, ph, err), err)) return rc;
    if (int rc = d2g_plan_err(ctx, d2g_plan_check_tail(in, err), err)) return rc;
    D2G_HIP(ctx, hipSetDevice(ctx->device));
    const size_t nblk = ph.bg.size();
    if (!use_ingested)
        if (int rc = sk->d_packed.grow(ctx, std::max<size_t>(in.packed_bytes, 4), 4096)) return rc;
    const PlanLayout lay = d2g_plan_layout(in.nrun, nblk);
    if (int rc = sk->d_arena.grow(ctx, lay.total, 65536)) return rc;
    if (int rc = sk->h_arena.grow(ctx, lay.total, 65536)) return rc;
    d2g_plan_fill(sk->h_arena, lay, in, ph);
    hipStream_t s = sk->stream;
    D2G_HIP(ctx, hipMemcpyAsync(sk->d_arena, sk->h_arena, lay.total, hipMemcpyHostToDevice, s));
    if (in.packed && in.packed_bytes) {
        // pageable source: stage through our own pinned buffer (the runtime would otherwise pin the
        // caller's pages on the fly, which contends with parser threads on the process' mm locks)
        if (int rc = sk->h_stage.grow(ctx, in.packed_bytes, 65536)) return rc;
        std::memcpy(sk->h_stage, in.packed, in.packed_bytes);
        D2G_HIP(ctx, hipMemcpyAsync(sk->d_packed, sk->h_stage, in.packed_bytes, hipMemcpyHostToDevice, s));
    }
    *out = KmerBatch{ctx, s, d2g_plan_kmer_args(sk->d_arena, lay, sk->d_packed, in.k, in.canon, in.w, in.alphabet), nblk, caller, &sk->k3};
    out->runs.packed = nullptr; out->runs.packed_bytes = 0; out->runs.w = in.w; out->runs.alphabet = in.alphabet;
    d2g_filter_args(sk->filter, &out->km);
    return D2G_OK;
}

void d2g_warm_k1() {
    hipFuncAttributes a;
    (void)hipFuncGetAttributes(&a, reinterpret_cast<const void *>(&k1_oph_kernel<true, true, false>));
    (void)hipFuncGetAttributes(&a, reinterpret_cast<const void *>(&k1_oph_count_kernel<true, true, false>));
    (void)hipFuncGetAttributes(&a, reinterpret_cast<const void *>(&k1_oph_kernel<true, true, true>));     // the filtered forms live in this code object too
    d2g_warm_filter();
}
