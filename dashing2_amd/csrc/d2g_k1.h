// d2g_k1.h -- host-side pieces shared by K1 (OPH) and K3 (k-mer counting + BagMinHash): the
// launch plan over a packed run stream and the persistent sketcher's staging buffers.
#pragma once
#include "d2g_kmers.h"
#include <vector>

// the plan unit's checks for a caller with a context: a refusal's text goes to last_error
inline int d2g_plan_err(d2g_ctx *ctx, int rc, const std::string &err) {
    if (rc) ctx->last_error = err;
    return rc;
}

// K1f: the k-mers of a --filterset input as an open-addressing table of raw 2-bit k-mers in device memory (d2g_filter.hip)
struct d2g_kmer_filter {
    d2g_ctx *ctx = nullptr;
    int k = 0, canon = 0;
    int w = 0;                                 // the window it was built under, 0 = none (never a value <= k)
    int alphabet = 0;                          // the alphabet its keys were encoded under (D2G_ALPHABET_*)
    uint64_t noccurrences = 0;                 // k-mers put in, duplicates counted (the reference's data_.size())
    uint64_t slots = 0;                        // a power of two >= 2 * noccurrences (>= 16)
    d2g_dev<uint64_t> d_tab;                   // [slots] keys, then [0] the all-ones flag, [1] the distinct keys in the slots
};
// the filter a plan or sketcher carries must fit the call: same context, alphabet, k, canon and window (nullptr fits everything)
int d2g_filter_check(d2g_ctx *ctx, const d2g_kmer_filter *f, int k, int canon, int w, int alphabet);
// a window as the library keeps it: w when w > k, else 0
inline int d2g_window_norm(int k, int w) { return w > k ? w : 0; }
// table pointer, mask and shift into the walker's arguments (nullptr: no filter); the caller has run d2g_filter_check
void d2g_filter_args(const d2g_kmer_filter *f, KmerArgs *km);
// K3 lays its key regions out from the k-mers per genome, which a filter makes data: one walk of the launch plan counts the
// survivors of every genome (host array [n]); synchronises `s`
int d2g_filter_survivors(d2g_ctx *ctx, const KmerArgs &km, size_t nblk, size_t n, uint64_t *out, hipStream_t s);

struct d2g_oph_plan {
    d2g_ctx *ctx = nullptr;
    const d2g_kmer_filter *filter = nullptr;   // VIEW (d2g_oph_plan_set_filter)
    int k = 0;
    int w = 0;                                 // d2g_oph_plan_create_windowed: the chunks are window positions (0 = none)
    int alphabet = 0;                          // d2g_oph_plan_create_alphabet: the stream is one byte per residue (0 = DNA)
    size_t n = 0, nrun = 0, nblk = 0;
    uint64_t nkmers = 0, nbases = 0;
    std::vector<uint32_t> h_run_len;           // host copies kept for K3's bucket layout
    std::vector<uint64_t> h_genome_run_off;
    PlanLayout lay;                            // the eight launch tables: pieces of ONE device buffer, as the sketcher ships them
    d2g_dev<uint8_t> d_arena;
    // the tables K3 lays its buckets out from (host copies; no stream: a plan is applied to any)
    PackedRuns runs(int canon) const { return {nullptr, 0, nullptr, h_run_len.data(), nrun, h_genome_run_off.data(), n, k, canon, w, alphabet}; }
};

// THE single constructor of the arguments a walker sees, and what d2g_km_protein() (d2g_kmers.h) rests on: a DNA batch stores canon
// as 0 or 1 here -- whatever non-zero value the caller passed; the kernels only ever asked `canon != 0` -- and a protein batch stores
// its alphabet's size (>= 6) in the same word.  Every KmerArgs that reaches a walking kernel is a copy of one made here.
// the ONLY place that points a walker's arguments at launch tables: `arena_dev` holds them as `lay` says (d2g_plan_fill)
inline KmerArgs d2g_plan_kmer_args(const uint8_t *arena_dev, const PlanLayout &lay, const uint8_t *packed_dev, int k, int canon, int w, int alphabet) {
    KmerArgs a{};
    auto u64 = [&](size_t at) { return reinterpret_cast<const uint64_t *>(arena_dev + at); };
    auto u32 = [&](size_t at) { return reinterpret_cast<const uint32_t *>(arena_dev + at); };
    a.packed = reinterpret_cast<const uint32_t *>(packed_dev);
    a.run_start = u64(lay.run_start); a.run_len = u32(lay.run_len); a.run_chunk_off = u64(lay.run_chunk_off);
    a.blk_genome = u32(lay.blk_genome); a.blk_chunk0 = u64(lay.blk_chunk0); a.blk_nchunks = u32(lay.blk_nchunks);
    a.blk_run_lo = u32(lay.blk_run_lo); a.blk_run_hi = u32(lay.blk_run_hi);
    a.k = k; a.canon = canon != 0; a.blk0 = 0; a.q = (uint32_t)d2g_window_q(k, w);
    if (alphabet != D2G_ALPHABET_DNA) a.canon = d2g_alphabet_size(alphabet);               // K1a: A (>= 6) where canon (0 here) stands; the kernels read it as asize
    return a;
}
// Host ingest feeds K1 in groups of inputs; re-allocating device buffers and uploading eight
// small tables per group costs ~20 ms, the kernel ~0.1 ms.  The sketcher keeps grow-only device
// buffers and ships all launch tables in ONE copy from a pinned arena.
struct d2g_k3_state;
struct d2g_k0_state;
struct d2g_sketcher {
    d2g_ctx *ctx = nullptr;
    const d2g_kmer_filter *filter = nullptr;               // VIEW (d2g_sketcher_set_filter)
    int w = 0;                                             // d2g_sketcher_set_window: every run walks minimizers when w > its k
    int alphabet = 0;                                      // d2g_sketcher_set_alphabet: every run reads a byte-per-residue stream (0 = DNA)
    d2g_stream stream;
    d2g_dev<uint8_t> d_packed;                             // grow-only, like the buffers below
    d2g_dev<uint64_t> d_regs;
    d2g_dev<uint32_t> d_counts;                            // d2g_sketcher_run_counts: one u32 per register
    d2g_dev<uint8_t> d_arena; d2g_pinned<uint8_t> h_arena; // the launch tables: device copy and its pinned source
    d2g_pinned<uint8_t> h_stage;                           // pinned staging of the packed stream
    d2g_k3_state *k3 = nullptr;                            // --multiset work buffers (d2g_k3.h)
    d2g_k0_state *k0 = nullptr;                            // device FASTA ingest (d2g_k0.hip): raw bytes, tile tables, the last run table
};
// an entry point's view of its arguments carries no window and no alphabet: the sketcher's, as the plan unit and the accounting in
// front of a stage see them
inline PackedRuns d2g_sketcher_view(const d2g_sketcher *sk, PackedRuns in) { in.w = d2g_window_norm(in.k, sk->w); in.alphabet = sk->alphabet; return in; }
void d2g_k0_state_destroy(d2g_k0_state *st);
bool d2g_k0_ingested(const d2g_sketcher *sk, uint64_t *nbases);   // d_packed holds a stream ingested by K0 (and how many bases)
void d2g_k0_invalidate(d2g_sketcher *sk);


// One batch of genomes ready for a walker: all that an operation behind a front door (K1, K1b, K3, the filter build, the screen)
// takes.  A view; exactly two functions make one, and each refuses before it touches the device.
struct KmerBatch {
    d2g_ctx *ctx = nullptr;
    hipStream_t s = nullptr;
    KmerArgs km{};                             // launch tables and packed stream on the device, the attached filter applied
    size_t nblk = 0;                           // workgroups of the walk
    PackedRuns runs{};                         // the host run tables (packed == nullptr), the window in runs.w: K3's layout
    d2g_k3_state **k3 = nullptr;               // where the K3 work state of this batch's owner lives: &sk->k3 or &ctx->k3
};
// a plan applied to a device stream on the caller's stream.  Refuses, in this order and before the first HIP call: a plan of
// another context, a stream that is not 4-byte aligned, a null stream under a plan with blocks, a filter that does not fit
// (d2g_filter_check).  The ONLY reader of a plan's launch tables.
int d2g_plan_batch(d2g_ctx *ctx, const d2g_oph_plan *plan, const uint8_t *packed_dev, int canon, void *stream, KmerBatch *out);
// validate + upload one batch (launch tables in one pinned-arena copy, packed stream through the pinned stage) on sk->stream;
// `ph_out` (if given) receives the plan.
// in.packed == nullptr: the stream d2g_sketcher_ingest_fasta left in the device buffer is used as it is.
int d2g_sketcher_stage(d2g_sketcher *sk, const PackedRuns &in, KmerBatch *out, PlanHost *ph_out);

// K3o (d2g_k3_bmh.hip) behind the min-count entry points of d2g_k1.hip: `regs_dev` [n][m] is pre-set to ~0 on the batch's stream;
// lowers the registers over the k-mers seen at least `mincount` (>= 2) times, waits for the status word
int d2g_k3_ophmin(const KmerBatch &b, uint64_t xormask, size_t m, uint32_t mincount, uint64_t *regs_dev);

// A host-pointer one-shot is the sketcher form on a sketcher that lives for one call: f(sk), and the sketcher goes on every path.
template <class F> int d2g_with_sketcher(d2g_ctx *ctx, F &&f) {
    if (!ctx) return D2G_ERR_INVALID;
    d2g_sketcher *sk = nullptr;
    if (int rc = d2g_sketcher_create(ctx, &sk)) return rc;
    const std::unique_ptr<d2g_sketcher, void (*)(d2g_sketcher *)> owner(sk, d2g_sketcher_destroy);
    return f(sk);
}
