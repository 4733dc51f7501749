// d2g_plan.h -- the sketch side's input and its launch plan, on the host alone: no HIP header and no d2g_ctx in here, so the
// grid arithmetic that the kernels trust runs under the host sanitizers (selftest/host_selftest.cpp) as it runs in libd2g.
#pragma once
#include "../../include/d2g.h"
#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

constexpr int K1_THREADS = 256;
constexpr int K1_CHUNK = 64;          // k-mers per lane-chunk
constexpr int K1_CPT = 4;             // chunks per lane (16 measured 3% slower: fewer, longer workgroups)
constexpr int K1_BLOCK_CHUNKS = K1_THREADS * K1_CPT;

// one batch of genomes as the caller's HOST arrays (a view: nothing is owned): 2-bit packed bases, the runs of valid bases in
// them and the runs of every genome.  What every sketch entry point takes; an entry point without a stream leaves packed null.
struct PackedRuns {
    const uint8_t *packed; size_t packed_bytes;     // 4 bases per byte, with 64 readable bytes behind the last base of any run
    const uint64_t *run_start;                      // [nrun] first base
    const uint32_t *run_len;                        // [nrun] bases, >= k
    size_t nrun;
    const uint64_t *genome_run_off;                 // [n + 1] genome g owns runs [genome_run_off[g], genome_run_off[g + 1])
    size_t n;
    int k, canon;
    int w = 0;                                      // -w: only the minimizer of every window of w bases is walked; <= k (0 included): every k-mer
    int alphabet = 0;                               // K1a: a protein D2G_ALPHABET_* reads `packed` as ONE BYTE per residue (its code); starts and
                                                    // lengths then count residues, canon must be 0 and there is no window
};

// K1w.  The widest window: q = w - k + 1 <= D2G_WINDOW_MAX_Q k-mers per window (include/d2g.h; a wider one is D2G_ERR_UNSUPPORTED)
// k-mers per window of a call, 1 without a window
inline int d2g_window_q(int k, int w) { return w > k ? w - k + 1 : 1; }
// THE number of k-mers a run of `len` valid bases emits: its k-mers, or with a window (w > k) its window positions; 0 for a run
// shorter than the span.  Chunks, blocks, K3's key regions, the screen's fed counts and every reported total follow from this.
inline uint64_t d2g_run_emissions_of(uint64_t len, int k, int w) {
    const uint64_t span = (uint64_t)(w > k ? w : k);
    return len >= span ? len - span + 1 : 0;
}

// launch plan: chunks of 64 emissions (k-mers, or window positions) per run, <= K1_BLOCK_CHUNKS chunks of ONE genome per workgroup.
// A run with k <= len < w emits nothing and owns no chunk.
struct PlanHost {
    std::vector<uint64_t> chunk_off, bc0;           // [nrun + 1] exclusive prefix of chunks per run; per workgroup its first chunk,
    std::vector<uint32_t> bg, bn, blo, bhi;         // its genome, its chunks and the runs [blo, bhi) that own one of them
    uint64_t nkmers = 0, nbases = 0;                // nkmers: emissions
};
// Each returns a D2G_* status and, with a refusal, its text in `err` (a caller with a context copies it to last_error).
// The plan of `in` (its tables only: packed is not looked at).  The kernels index with what this writes and check nothing.
int d2g_plan_build(const PackedRuns &in, PlanHost &p, std::string &err);
// packed_bytes >= (max(run_start + run_len) + 3) / 4 + 64 (a protein alphabet: max(run_start + run_len) + 64, a byte per symbol):
// all that keeps the walker's window reads (up to 20 bytes past a chunk's first word) inside the buffer
int d2g_plan_check_tail(const PackedRuns &in, std::string &err);
// the counting forms with host outputs return uint32 counts without the reference's wrap (idcounts() copies doubles into
// uint32, oph.h:272-277): a genome that could reach 2^32 emissions is refused.  Tables that d2g_plan_build will reject (null, not
// monotone, a run shorter than k) pass: they are left to it.
int d2g_plan_check_count_range(const PackedRuns &in, std::string &err);

// the eight launch tables as 256-byte-aligned pieces of ONE buffer: byte offsets and the buffer's size
struct PlanLayout {
    size_t run_start, run_chunk_off, blk_chunk0, run_len, blk_genome, blk_nchunks, blk_run_lo, blk_run_hi, total;
};
PlanLayout d2g_plan_layout(size_t nrun, size_t nblk);
// the tables of `in` and its plan `p` into a host buffer of lay.total bytes, lay = d2g_plan_layout(in.nrun, p.bg.size())
void d2g_plan_fill(uint8_t *arena, const PlanLayout &lay, const PackedRuns &in, const PlanHost &p);
