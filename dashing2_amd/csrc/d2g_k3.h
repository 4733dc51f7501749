// d2g_k3.h -- the host side that the units of K3 (the --multiset path) share: the work state in parts by owner, the run a staged
// batch goes through, the status word, and the few host functions one unit offers the others.  A kernel is launched only from the
// unit that defines it.
//   d2g_k3_bucket.hip       layout, the multi-split of the keys into buckets (k3_* / k3c_* hist, scan, scatter, refine), k3_begin
//   d2g_k3_bmh.hip          exact counts in LDS tables, BagMinHash over them (main / survivor / verify), K3o, K3Run::run
//   d2g_k3_lists.hip        BagMinHash over explicit (id, weight) lists: the list stage below, d2g_bmh_from_weighted*, d2g_bmh_device_lists
//   d2g_k3_sets.hip         K3s: the exact sets in sorted form (ks_*)
//   d2g_k3_countsketch.hip  K3k: the count-sketch chain (k3k_*)
#pragma once
#include "d2g_k1.h"
#include "d2g_countsketch.h"
#include <vector>

constexpr int K3_THREADS = 256;

enum K3Status : int {         // the device status word (d_status[0]): 0 until a kernel raises it
    K3_TABLE_OVERFLOW = 1,    // a round's keys did not fit the LDS count table
    K3_BAD_WEIGHT = 2,        // a weight outside (0, 2^53] (explicit weighted sets)
    K3_STACK_OVERFLOW = 3,    // the BagMinHash descent ran out of its private stack
    K3_REGION_OVERFLOW = 4,   // a survivor region of the light first pass filled up: the host repeats the pass in the heavy form
    K3_SORT_OVERFLOW = 5,     // K3s: a sort range holds more keys than its LDS stage (keys that share their top bits: not hashes)
};
// (d2g_k3_bmh.hip) a final status word as the library's error: code and message; the word of a state read on `s` (waits) and mapped
int k3_status_error(d2g_ctx *ctx, int status);
int k3_check_status(d2g_ctx *ctx, d2g_k3_state *st, hipStream_t s);

inline uint32_t ceil_log2(uint64_t x) { uint32_t b = 0; while ((1ull << b) < x) ++b; return b; }

// ---- the list stage (d2g_k3_lists.hip): BagMinHash over (id, weight) lists that lie in device memory, set i = elements
// [set_off[i], set_off[i + 1]).  The workgroup tables of one walk and the host arrays they are uploaded from; grow-only.  Its owner
// keeps it until the stream of the walk has been waited for: the uploads are asynchronous.
struct K3ListTables {
    d2g_dev<uint64_t> lo;            // [nb] first element of workgroup b
    d2g_dev<uint32_t> set;           // set [nb], then cnt [nb]
    d2g_ws_blocks wb;
    std::vector<uint64_t> guess;
};
// the caller's device buffers of the sets walked (slices of larger ones, or a one-shot call's own)
struct K3ListRegs {
    uint64_t *h;                     // [ng][m] registers, +inf
    uint64_t *guess;                 // [ng]
    uint32_t *redo;                  // [ng]
    double *tw;                      // [ng]
    int *status;                     // [2] status word and redo counter, zero
};
// what prepare leaves for walk
struct K3ListWalk { const uint64_t *ids; const double *w; const K3ListTables *t; K3ListRegs r; size_t ng, nb, m; };
// prepare: the totals tw [ng] (host) keep the bound finite, or D2G_ERR_INVALID; first guesses and workgroup tables from set_off [ng + 1]
// (host) and the totals, both uploaded on `s` with the totals themselves (r.tw: AFTER the registers were initialised, which zeroes it).
// walk: every set under its guess, the verification, the failed sets again under a guess 16 times larger, until none is left; waits
// for `s` once per pass and maps the status word.  After a failure of either the caller waits for `s` before its host arrays go.
int k3_lists_prepare(d2g_ctx *ctx, hipStream_t s, const uint64_t *ids_dev, const double *w_dev, const uint64_t *set_off, const double *tw,
                     size_t ng, size_t m, K3ListTables &t, const K3ListRegs &r, K3ListWalk *out);
int k3_lists_walk(d2g_ctx *ctx, hipStream_t s, const K3ListWalk &p);

// ---- grow-only work buffers of the --multiset path (owned by a sketcher or by a one-shot call), in parts by owner.  A unit writes its
// own part; K3s reads the counting part's output, K3k and the sketch share the sketch part's registers.
struct d2g_k3_state {
    struct Counting {                    // d2g_k3_bucket.hip lays out and fills, d2g_k3_bmh.hip counts
        d2g_dev<uint32_t> d_gtab;        // g_bbits [n] + g_boff [n+1]
        d2g_dev<uint64_t> d_koff;        // [n+1]
        d2g_dev<uint32_t> d_bucket_cnt;
        d2g_dev<uint64_t> d_bucket_off;
        d2g_dev<uint64_t> d_cursor;
        d2g_dev<uint32_t> d_l2;          // two-level split: coarse bucket table
        d2g_dev<uint32_t> d_blk_coarse;
        d2g_dev<uint64_t> d_keys;
        d2g_dev<uint64_t> d_skeys;       // big inputs: keys regrouped by sub-range
        d2g_dev<uint32_t> d_gblk;        // compact path: first launch-plan block of each genome
        d2g_dev<uint16_t> d_tile_cnt;
        d2g_dev<uint32_t> d_tile_off;
        d2g_dev<uint64_t> d_sub_off;
        d2g_dev<uint32_t> d_gsplit;
        d2g_dev<uint64_t> d_gsub;
        d2g_dev<int> d_status;           // [0] status, [1] nredo
        d2g_dev<uint32_t> d_out_counts;
        d2g_dev<uint32_t> d_bucket_nd;
        d2g_dev<uint64_t> d_out_keys;
    } count;
    struct Sketch {                      // d2g_k3_bmh.hip; K3k walks its lists into d_h / d_tw / d_guess / d_redo by slices
        d2g_dev<uint64_t> d_h;
        d2g_dev<double> d_tw;
        d2g_dev<uint64_t> d_guess;
        d2g_dev<double> d_tw_bucket;
        d2g_dev<uint32_t> d_redo;
        d2g_dev<uint64_t> d_gq;          // survivors of the light first pass (QEntry)
        d2g_dev<uint64_t> d_gq_off;      // [grid+1] region offsets, then [grid] u32 counts
        d2g_stream xs;                   // second stream of the sub-batch pipeline
        d2g_event ev_a[8], ev_b;
    } sketch;
    struct Sets {                        // K3s, the sorted emission (d2g_k3_sets.hip)
        d2g_dev<uint32_t> d_ks_pbits;    // [n] log2(sort ranges) of genome g
        d2g_dev<uint64_t> d_ks_rbase;    // [n+1] first sort range of genome g
        d2g_dev<uint32_t> d_ks_cnt;      // [nranges]
        d2g_dev<uint64_t> d_ks_off;      // [nranges+1]
        d2g_dev<uint64_t> d_ks_cur;      // [nranges]
        d2g_dev<uint64_t> d_ks_setoff;   // [n+1]
        d2g_dev<uint64_t> d_ks_cards;    // [n][2]
        d2g_dev<uint64_t> d_ks_keys;     // host-pointer form: the sorted keys ...
        d2g_dev<uint32_t> d_ks_counts;   // ... and counts (also the count column of a caller that asked for keys only)
    } sets;
    struct CountSketch {                 // K3k, the count-sketch (d2g_k3_countsketch.hip)
        d2g_dev<int32_t> d_cs_table;     // [rows of one group][cells], zeroed per group for exactly rows * cells cells
        d2g_dev<uint32_t> d_cs_row;      // [n] the table row of genome g inside its group
        d2g_dev<uint32_t> d_cs_tile_cnt; // [rows * tiles] cells kept per tile of K3K_TILE cells
        d2g_dev<uint64_t> d_cs_tile_off; // [rows * tiles + 1] their exclusive prefix, then row_off [rows + 1], then the total weight [rows]
        d2g_dev<uint64_t> d_cs_ids;      // the lists of one group: cell numbers, each row's ascending ...
        d2g_dev<double> d_cs_w;          // ... and |count|
        K3ListTables lists;              // BagMinHash over them
    } cs;
};

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
// (d2g_k3_bucket.hip) everything that follows from kh.gk: buckets, key offsets, sub-ranges
int k3_layout_buckets(d2g_ctx *ctx, size_t n, K3Host &kh);

// registers and total weights (R12) / distinct (key, count) per bucket (R11) / their number only / One-Permutation registers over the
// k-mers counted at least thr + 1 times (K3o)
enum class K3Mode { Sketch, Count, Distinct, OphMin };

// count (R11) or sketch (R12) of one staged batch: what the caller fills in, and the stages
struct K3Run {
    d2g_ctx *ctx = nullptr; d2g_k3_state *st = nullptr; hipStream_t s = nullptr;
    KmerArgs km; size_t nblk = 0;      // the launch plan of the staged batch
    K3Host kh; size_t n = 0;           // its bucket layout (k3_layout); genomes
    uint64_t xormask = 0; size_t m = 1; double thr = 0.;
    uint64_t key_words = 0;            // d_keys in 8-byte words: a masked key per k-mer on the generic path, a 4-byte stored word on the compact one
    uint64_t *oph_regs = nullptr;      // OphMin: the caller's registers [n][m] (device), pre-set to ~0 on this stream
    int run(K3Mode mode);                                                       // d2g_k3_bmh.hip: buckets, then the mode's stages
    int upload_tables(), bucket_prepare(), bucket(size_t g_lo, size_t g_hi);    // d2g_k3_bucket.hip
    std::vector<size_t> subbatches(K3Mode mode) const;
};
// (d2g_k3_bucket.hip) what every K3 operation begins with: the work state of the batch's owner (made on first use), the run filled
// from the batch, the bucket layout
int k3_begin(const KmerBatch &b, K3Run &r);
// (d2g_k3_bmh.hip) registers to +inf, weights and redo flags to zero; the checks of a BagMinHash call in front of its batch; the exact
// (key, count) of every bucket of a begun run (n > 0), left in the counting part: what the count and both set forms read
void k3_init_registers(hipStream_t s, uint64_t *h, size_t nh, double *tw, uint32_t *redo, size_t n);
int bmh_check(d2g_ctx *ctx, size_t n, size_t sketchsize, double count_threshold, const double *sig_out, const double *total_weight_out);
int k3_exact_counts(K3Run &r, uint64_t xormask, double count_threshold);

// one per unit: d2g_warm_k3 (d2g_k3_bmh.hip) loads its own code object and calls these
void d2g_warm_k3_bucket(); void d2g_warm_k3_lists(); void d2g_warm_k3_sets(); void d2g_warm_k3_countsketch();
