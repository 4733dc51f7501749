// d2g_k2.h -- internal: the prepared comparison operand shared by the K2 translation units.
#pragma once
#include "d2g_internal.h"

#include <algorithm>

// part of an upper-triangle launch's fill, carried by a kernel of the prepare chain: the workgroups from `own` on write pieces
// piece0 .. of 32 KB each (own = 0xFFFFFFFF: nobody rides)
struct SpRider { uint32_t *out; size_t cnt; const uint32_t *vsrc; uint32_t vimm, own, piece0; };
constexpr SpRider SP_NO_RIDER{nullptr, 0, nullptr, 0u, 0xFFFFFFFFu, 0u};
constexpr int SP_FILL_PER_THREAD = 8, SP_FILL_THREADS = 256;   // sp_fill_kernel: a workgroup writes one piece of 32 KB
inline size_t sp_fill_pieces(size_t cnt) { return div_up<size_t>(cnt / 4 + 1, (size_t)SP_FILL_THREADS * SP_FILL_PER_THREAD); }
// ---- riders (sp_ride): the share of an announced output's fill that one hosting kernel of the prepare chain carries, in parts of SP_RW_ALL; the
// last host (place) takes what is left.  Classic schedule: the hosts' own durations at config 3 (us) -- column plan, flatten, count, attach and scan are
// one to forty workgroups on an idle chip and each hides about what it lasts.  Merged schedule (d2g_bitslice_prepare): the hosts of bits 1 and 2 are the
// launches that CONTAIN the column plan (link pass 0) and flatten (the planes body); they last ~20 and ~17 us but stream the ids themselves, so their
// shares are not their durations but what was fitted on the GPU (profiles/k2_merged_prepare.txt section 4): the step is flat between 3 and 8 parts for
// either of them, and 2 us slower with 12 parts on the link launch or with fewer than ~8 on the two together (the rest lands on place).
// Schedule 2 (the planes behind emit's workgroups): bit 2's host is flatten alone again, forty workgroups; it keeps SP_RW_M_PLANES -- NOT re-fitted
// (profiles/k2_planes_emit.txt says so); emit, the planes' new host, carries no riders.
#ifndef D2G_SP_RW_M_LINK0
#define D2G_SP_RW_M_LINK0 8
#endif
#ifndef D2G_SP_RW_M_PLANES
#define D2G_SP_RW_M_PLANES 5
#endif
constexpr unsigned SP_RW_PLAN = 6, SP_RW_FLATTEN = 5, SP_RW_COUNT = 5, SP_RW_ATTACH = 5, SP_RW_SCAN = 8, SP_RW_ALL = 35;
constexpr unsigned SP_RW_M_LINK0 = D2G_SP_RW_M_LINK0, SP_RW_M_PLANES = D2G_SP_RW_M_PLANES;
// The FAST rank kernel (bs_rank_kernel<false, true>: N <= 12 288) is no host of rider workgroups -- every wave slot of the chip is taken for its 52 us at
// config 3 -- but its HBM is almost idle, and a store needs no wave slot: its own threads write the FIRST pieces of the fill between their probe chains
// (bit 64 of D2G_SP_RIDE).  Its share in parts of SP_RW_ALL is d2g_k2_tuning::rank_share (D2G_SP_RANK_SHARE; fitted: profiles/k2_rank_fill.txt);
// SP_RANK_FILL_PER_WG = what one workgroup can hold: one 16-byte store per thread and iteration of its claim loop.  What is left goes to the six hosts by
// the weights above.
constexpr int BS_RANK_THREADS = 1024, BS_RANK_PF = 12;          // bs_rank_kernel: threads of a workgroup; values a FAST thread keeps in registers
constexpr uint32_t SP_RANK_FILL_PER_WG = (uint32_t)(BS_RANK_PF * BS_RANK_THREADS * 16 / (SP_FILL_THREADS * SP_FILL_PER_THREAD * 16));   // = 6 pieces
static_assert(SP_RANK_FILL_PER_WG * SP_FILL_THREADS * SP_FILL_PER_THREAD == BS_RANK_PF * BS_RANK_THREADS, "the rank kernel's stores of one workgroup are whole pieces");

// start-of-prepare work of the sparse path's ordering, carried by a kernel that runs anyway (k2_transpose_kernel for a set that owns its operand,
// sp_unpack_kernel for the multi-GPU engine's gathered one) instead of a launch and memsets of its own: label[j] = j, `owords` words at `ones` set to
// all-ones (the hints), `zwords` words at `zero` cleared (counters, linked flags, tile bitmap + control words, order words, the pair list's cursor).
// Nothing between that kernel and the first link pass touches these arrays (the rank kernel and the first look's two kernels have buffers of their own).
struct SpInit {
    uint32_t *label = nullptr, *ones = nullptr, *zero = nullptr;
    uint32_t n = 0, owords = 0, zwords = 0;
};
#ifdef __HIPCC__
__device__ __forceinline__ void sp_init_part(const SpInit &si, size_t lin, size_t nthreads) {
    if (!si.label) return;
    if (lin < si.n) si.label[lin] = (uint32_t)lin;
    for (size_t x = lin; x < si.owords; x += nthreads) si.ones[x] = 0xFFFFFFFFu;
    for (size_t x = lin; x < si.zwords; x += nthreads) si.zero[x] = 0;
}
#endif

// the output of the NEXT upper-triangle launch, announced ahead of the prepare (d2g_cmp_ut_announce_dev): the prepare's latency-bound
// kernels (column plan, flatten, count, attach, scan, place: one to forty workgroups each) carry the fill as extra workgroups
struct SpAnnounced {
    uint32_t *out = nullptr; size_t cnt = 0; const uint32_t *vsrc = nullptr; uint32_t vimm = 0;   // the fill value = Store::value_from_mismatches(S, S): the count 0 (vsrc null), or lut[0] (read by the riders when they run)
    uint32_t next = 0, total = 0;   // pieces of 32 KB handed out so far / in all (0: nothing rides in this prepare)
    int mask = 0;                   // D2G_SP_RIDE: the kernels of this prepare that may carry pieces
    void announce(uint32_t *o, size_t n, const uint32_t *src) { out = o; cnt = n; vsrc = src; vimm = 0; }
    void cancel() { out = nullptr; }                  // nothing rides on the next prepare
    void served() { out = nullptr; total = 0; }       // an announcement serves ONE prepare
    // a prepare starts: every piece rides on it, or none (`carry` false: not the sparse path, or the launch will be dense and fill nothing; more pieces than a grid holds)
    void begin(int ride_mask, bool carry) {
        mask = ride_mask; next = 0;
        const size_t pieces = sp_fill_pieces(cnt);
        total = (out && carry && mask && pieces <= 0x7FFFFFFFu) ? (uint32_t)pieces : 0u;
    }
    uint32_t riding() const { return total; }         // pieces this prepare carries
    SpRider take_all() { next = total; return SpRider{out, cnt, vsrc, vimm, 0u, 0u}; }   // a fill kernel of its own writes every piece: nothing left for the riders
    // the FAST rank kernel's share (bit 64 of the mask), asked for BEFORE any host: the first pieces [0, *n), at most `cap` (what its grid holds).  What the
    // riders and the launch see is the same prefix bookkeeping as without it
    SpRider take_first(unsigned weight, uint64_t cap, uint32_t *n) {
        *n = 0;
        if (next != 0 || !total || !(mask & 64)) return SP_NO_RIDER;
        *n = (uint32_t)std::min<uint64_t>(std::min<uint64_t>(total, cap), ((uint64_t)total * weight + SP_RW_ALL - 1) / SP_RW_ALL);
        next = *n;
        return SpRider{out, cnt, vsrc, vimm, 0u, 0u};
    }
    // the share of a hosting kernel with `own` workgroups of its own (bit `bit` of the mask): `grid` = what to launch
    SpRider take(unsigned own, unsigned weight, bool last, int bit, unsigned *grid) {
        *grid = own;
        if (next >= total || !(mask & bit)) return SP_NO_RIDER;
        const uint32_t left = total - next;
        uint32_t n = last ? left : (uint32_t)std::min<uint64_t>(left, ((uint64_t)total * weight + SP_RW_ALL - 1) / SP_RW_ALL);
        n = std::min<uint32_t>(n, 0x7FFFFFFFu - own);
        const SpRider r{out, cnt, vsrc, vimm, own, next};
        next += n;
        *grid = own + n;
        return r;
    }
};

// what is already written of the output of the next upper-triangle launch: by the engine at the start of its step (d2g_bitslice_prefill), or by
// the riders of a prepare.  The next sparse launch skips that part of its fill.
struct SpFilled {
    uint32_t *out = nullptr;            // the output (null: nothing is filled)
    size_t cnt = 0;                     // ... how many outputs that fill covered
    size_t pieces = 0;                  // ... how many 32 KB pieces of it are written (all of them after an early fill; what rode on the prepare's kernels otherwise)
    const uint32_t *src = nullptr;      // ... WHAT was written: the table whose first entry is the fill value (nullptr: the count 0)
    bool by_riders = false;             // ... by the riders of a prepare (void once another prepare has run) or by d2g_cmp_ut_prefill_dev (valid until the next upper-triangle launch)
    void set_early(uint32_t *o, size_t n, const uint32_t *s) { out = o; cnt = n; pieces = (size_t)-1; src = s; by_riders = false; }
    void set_by_riders(const SpAnnounced &a) { out = a.out; cnt = a.cnt; pieces = a.next; src = a.vsrc; by_riders = true; }   // (the launch fills what is left)
    // pieces [0, done_for) of a launch's `npieces` need no fill.  ADVICE r5: the same output, the same rows AND the same fill value -- a count
    // launch into a buffer that was pre-filled for a table launch fills again
    size_t done_for(const uint32_t *o, size_t n, const uint32_t *s, size_t npieces) const { return (out == o && cnt == n && src == s) ? std::min(pieces, npieces) : 0; }
    void void_after_prepare() { if (by_riders) out = nullptr; }   // what an EARLIER prepare's riders wrote is void once another prepare has run (the caller may have used the buffer in between)
    void clear() { out = nullptr; }                   // a launch has written (or filled) every output itself
};

// the words of mapped host memory the device writes and the host reads without synchronisation (SpState::h_gaveup / d_gaveup):
//   GAVEUP     1 = the last ordering raised order[0] (the next prepare skips the ordering); the host writes it too, after a first look
//   LIST_LEN   length of the last prepare's pair list (the permute launch)
//   SUMS .. +3 the first look's raw sums E, F, shared values, planes (sp_sample_fin_kernel)
//   TICKET     the word the first look's last workgroup writes when the sums are in
enum SpMappedWord : uint32_t { SP_MW_GAVEUP = 0, SP_MW_LIST_LEN = 1, SP_MW_SUMS = 2, SP_MW_TICKET = 6, SP_MW_WORDS = 16 };

// which way a prepare goes: the first look at the matrix, the remembered give-up, the form of the pair list
struct SpDecision {
    unsigned prepares = 0; bool skipped = false;   // prepares so far; the last one skipped the ordering
    int merged = 0; unsigned kernels = 0;          // the last prepare: the schedule it ran -- 0 classic, 1 merged (planes beside flatten), 2 merged (planes behind emit) (d2g_bitslice_prepare); the kernels it enqueued, the transpose included (diagnostics)
    int skip_cached = -1;             // this prepare's reading of the remembered give-up (-1: not read yet)
    bool sample_pending = false; uint32_t sample_ticket = 0;   // the first look's kernels are enqueued; the value their last workgroup writes to the ticket word when the sums are in
    bool pred_valid = false, pred_dense = false; double pred_entries = 0, pred_family_pairs = 0;   // what the sample of THIS prepare says (valid until its ordering has been enqueued)
    bool big = true;                  // this prepare enqueued the binned form of the pair list (sp_expect_long_list)
    bool looked = false, looked_dense = false; uint32_t samp_sums[4] = {0, 0, 0, 0};   // the last prepare's first look: taken, its decision, its raw sums E, F, shared values, planes
    uint64_t fill_announced = 0, fill_rank = 0, fill_carried = 0;   // the last prepare: 32 KB pieces of the output announced to it / written by its rank kernel / by its other kernels (riders, side fill) -- d2g_cmp_set_fill_detail
};

// everything the sparse path of a set owns (sp_alloc builds one; a set without it takes the dense walk)
struct SpState {
    unsigned sp_launch = 0;       // sparse launches so far: the control words are double-buffered (a launch zeroes the next one's)
    d2g_dev<uint32_t> d_stream_s;   // plane stream in sorted order
    d2g_dev<uint32_t> d_sperm;      // [Nstride] sketch at sorted position p (0xFFFFFFFF = padding)
    d2g_dev<uint32_t> d_sinv;       // [Npad]    sorted position of sketch j
    d2g_dev<uint32_t> d_label;      // [2][Npad] union-find labels (-> segment starts after the sort) | root of every sketch
    d2g_dev<uint32_t> d_owner;      // [S][owner_stride] one holder of every shared value (rank r -> owner[r - 1]); single-partition owning sets only
    size_t owner_stride = 0;
    d2g_dev<uint32_t> d_segend;     // [Npad]    end of the segment of root r (the sort's scan)
    d2g_dev<uint32_t> d_posseg;     // [Npad][2] (start, end) of the segment sorted position p lies in (sp_place_kernel; the sub-tile test of the pair kernel and the pair list)
    d2g_dev<uint32_t> d_hint;       // [2][Npad] per sketch the smallest holder of a value it shares (even / odd column pairs), 0xFFFFFFFF = none
    d2g_dev<uint32_t> d_spz;        // ONE block the prepare clears: the arrays below
    size_t spz_words = 0;
    uint32_t *d_lcnt = nullptr;       // (this and d_gbm, d_order, d_plctl, d_fullctl, d_binc: inside d_spz) [Npad+1]  counting sort: sketches per root, then the placing cursors (= segment ends)
    uint32_t *d_gbm = nullptr;        // 8 control words + the tile bitmap over ALL sorted row blocks (the segments' tiles); partial launches derive theirs from it
    uint32_t *d_order = nullptr;      // [8] [0] 1 = the launches walk every tile of the caller's-order operand (dense), [2] deep label chains
    uint32_t *d_plctl = nullptr;      // [12] [0] entries emitted into the pair list
    d2g_dev<uint32_t> d_rowpos;     // [Nstride] launch rows: sorted position of launch row k
    d2g_dev<uint32_t> d_rowk;       // [Npad]    launch row of sketch j (0xFFFFFFFF = not a row of this launch)
    d2g_dev<uint32_t> d_rowstream;  // [planes][Nstride] row-coded words of the launch rows, gathered (partial launches)
    d2g_dev<uint32_t> d_tiles, d_spctl; uint32_t *d_tilebm = nullptr;   // a partial launch's work list, 2 x 8 control words {tiles listed, flags, -, candidates} + its tile bitmap (inside d_spctl)
    d2g_dev<uint32_t> d_tiles_full; uint32_t *d_fullctl = nullptr;   // work lists + control words (inside d_spz) of a whole-triangle launch, left by the prepare (sp_permute_kernel)
    bool full_list_valid = false;
    d2g_pinned<uint32_t> h_gaveup; uint32_t *d_gaveup = nullptr;   // SP_MW_WORDS words of mapped host memory (SpMappedWord) and their device address; no mapped memory: h_gaveup is null and d_gaveup a spare word of d_order
    d2g_stream fill_stream; d2g_event fill_fork, fill_join;   // a LARGE announced output is filled beside the rank kernel (d2g_bitslice_prepare)
    d2g_stream samp_stream; d2g_event samp_event;   // the first look runs beside the column plan and the planes kernel
    d2g_dev<uint32_t> d_samp;       // [16][Npad] + 2: the first look at a matrix (sp_sample): registers shared with sixteen sampled sketches
    SpDecision dec;
    SpAnnounced announced;
    SpFilled filled;
    const uint32_t *last_ctl = nullptr;   // control words of the last sparse launch (d2g_cmp_set_sparse_info)
    d2g_dev<unsigned long long> d_plist;   // pair list: (i | j << 32), i < j caller's indices, one entry per (pair in different segments, shared value)
    size_t plist_cap = 0;
    // the list BINNED by output region (band of 32 rows x chunk of 2^bin_cshift columns): what sp_compose_kernel reads
    d2g_dev<unsigned long long> d_plist2;
    uint32_t *d_binc = nullptr;                       // [nbins] entries per bin (inside the block the prepare clears)
    d2g_dev<uint32_t> d_bstart;                     // [nbins + 1] first entry of every bin in d_plist2
    d2g_dev<uint32_t> d_cw_ents; d2g_dev<unsigned long long> d_cw_vals; size_t cw_ecap = 0, cw_vcap = 0;   // sp_emit_kernel -> sp_pairs_kernel: the holders of the mixed values, one record per value
    d2g_dev<uint32_t> d_hoff;                       // [bin_nwg][nbins] where the entries a counting workgroup met go inside their bin (sp_hist_body -> sp_bin_kernel)
    uint32_t nbins = 0, bin_nch = 0, bin_cshift = 10, bin_nwg = 1;
    bool bin_ok = true;                               // the bins fit (sp_bin_geometry): otherwise the list is applied entry by entry only
    size_t tilebm_words = 0, tiles_cap = 0;
};

struct d2g_cmp_set {
    d2g_ctx *ctx = nullptr;
    size_t N = 0, S = 0;
    size_t Npad = 0;              // N rounded up to the column tile (256)
    int algo = D2G_CMP_DIRECT;    // algorithm actually prepared
    d2g_dev<uint64_t> d_rows;     // [N][S]     row-major 64-bit patterns
    d2g_dev<uint64_t> d_cols;     // [S][Npad]  register-major (transposed), zero padded
    // sets of truncated codes (algo == D2G_CMP_PLANES, d2g_k2_planes.hip): the only buffer of such a set
    d2g_dev<uint32_t> d_cplanes;  // [ntb][cplanes][Nstride]: bit t%32 of word (t/32, p, j) = bit (cplanes-1-p) of code (j, t)
    int cplanes = 0;              // bits per code: 8, 16 or 32
    // bit-sliced operand (algo == D2G_CMP_BITSLICE); all buffers are allocated once per set
    d2g_dev<uint32_t> own_planes, own_meta;   // what d_planes / d_meta point at when the set allocated them itself; empty in a set over the caller's operand
    uint32_t *d_planes = nullptr; // exchanged form [ntb][nbits_cap+1][Nstride]: bit x of word = bit b of id[32*tb+x][j], unique values
                                  // coded 0; last slot = the "unique" plane (fixed geometry: groups are independent)
    d2g_dev<uint32_t> d_stream;   // what the pair kernel walks: [live planes of all groups][2][Nstride] -- row-coded words, then the
                                  // same plane with unique values coded all-ones (column coding); + one block of slack
    size_t Nstride = 0;           // Npad + 64 (row tiles may read past Npad)
    int nbits_cap = 0;            // id-plane slots per 32-register group: smallest c with 2^c >= N/2 + 2
    int ntb = 0;                  // ceil(S/32)
    uint32_t *d_meta = nullptr;   // [tb] = max over the group's columns of (#values occurring >= 2 times) + 1 (device side; the kernels
                                  //       derive the live plane count from it, no host round trip)
    d2g_dev<uint32_t> d_ids;      // workspace: [S][Npad] dense ids (engine-managed gathered operands: allocated with d_colcnt for the sparse path, ids re-derived from the planes)
    int id_bits = 32;             // width of a word of d_ids: 16 where the set's rank kernel is single-partition (N <= 21 845) and D2G_BS_ID16 is on -- 0 = padding,
                                  // 0x8000 = unique, 1 .. 0x7FFF = rank -- 32 otherwise (MULTI / split ranks, ids unpacked from planes); d_ids then holds half as many words
    uint32_t T = 0; int logT = 0; // hash space of the rank kernel (power of two >= 1.5 N)
    bool borrowed = false;        // planes/meta are the caller's (d2g_cmp_set_from_planes_dev): never re-prepared, status from status_words
    bool want_exchange = false;   // d_planes is kept up to date by every prepare (set by the first export)
    // column plan (bs_colplan_kernel): the 32-register groups are formed from the columns SORTED by their live-plane class, so
    // that meta[tb] is the maximum over 32 similar columns (equality counts are a sum over columns: any permutation is exact)
    d2g_dev<uint32_t> d_colcnt;   // [S][BS_CC_STRIDE]: per column, slots 0..3 = rank offset of each split of the rank kernel, slot 4 = #shared values
    d2g_dev<uint32_t> d_perm;     // [ntb*32]: the column that sits in each register slot of the operand, ~0 = padding
    int nsplit = 1;               // workgroups per column in the multi-partition rank kernel (narrow slices of large N: fills the CUs)
    // exporter sets (the multi-GPU engine's per-rank column slices): the prepare writes the exchange form, the group meta and its
    // status word straight into the caller's gathered operand; no plane stream, no private d_planes
    bool export_only = false;
    uint32_t *ex_planes = nullptr, *ex_meta = nullptr, *ex_status = nullptr;
    // engine-managed gathered sets (d2g_allpairs): the engine derives the plane stream itself (per chunk, as the groups arrive) and
    // points the set at the status words every rank's prepare contributed
    bool managed = false;
    const uint32_t *status_words = nullptr; int n_status = 0;
    // ---- sparse tiles + pair list (d2g_k2_sparse.h).  The sketches are put in an order that makes a family -- sketches that agree in
    // many registers -- a run of adjacent positions, the plane stream is built in THAT order, and an upper-triangle launch walks only
    // the 32 x 256 tiles a family's rows and columns meet in; pairs of DIFFERENT families that share a value by chance are counted from
    // a pair list; every other pair has 0 matches (the output is pre-filled with the value of 0).  Exact for any input.
    std::unique_ptr<SpState> sp;  // everything that path owns; null: not eligible, switched off (D2G_BS_SPARSE, D2G_BS_SPARSE_MIN_N) or no memory for it -- the dense walk
    bool sparse_ok() const { return sp != nullptr; }
    size_t ncols = 0;             // register columns the sparse path walks: S, or all ntb * 32 register slots of an engine-managed gathered operand
    bool srt_valid = false;       // sp->d_stream_s / sp->d_sperm describe the operand last prepared
    mutable bool nat_valid = false;   // d_stream (caller's order; rectangular launches, dense launches) is up to date (mutable: a launch on a const set writes it on demand, d2g_bitslice_ensure_natural)
};
constexpr int BS_CC_STRIDE = 8;

struct PairShape;
int  finish_shape(d2g_ctx *ctx, PairShape &sh, unsigned rb);   // d2g_k2.hip

// d2g_k2_planes part (same shared object): (gt, lt) / equality counts of a set of truncated codes over one launch shape
int  d2g_planes_gtlt(d2g_ctx *ctx, const d2g_cmp_set *set, const PairShape &sh, uint32_t *gt, uint32_t *lt, hipStream_t s);
int  d2g_planes_eq(d2g_ctx *ctx, const d2g_cmp_set *set, const PairShape &sh, uint32_t *eq, hipStream_t s);

// d2g_k2_bitslice part (same shared object)
void d2g_bitslice_geometry(d2g_cmp_set *set);
int  d2g_bitslice_alloc(d2g_ctx *ctx, d2g_cmp_set *set);
int  d2g_bitslice_prepare(d2g_ctx *ctx, d2g_cmp_set *set, hipStream_t s);
int  d2g_bitslice_export(d2g_ctx *ctx, d2g_cmp_set *set, hipStream_t s);
int  d2g_bitslice_alloc_stream(d2g_ctx *ctx, d2g_cmp_set *set);
int  d2g_bitslice_ensure_natural(d2g_ctx *ctx, const d2g_cmp_set *set, hipStream_t s);   // caller's-order stream of a sparse set, on demand
// engine-managed gathered operands (d2g_mgpu.hip): buffers for the sparse-tile path, and the call that says "every group has arrived and
// its plane stream is derived": ids are re-derived from the planes, the sketches ordered, the sorted stream written
int  d2g_bitslice_managed_sparse_alloc(d2g_ctx *ctx, d2g_cmp_set *set);
int  d2g_bitslice_managed_ready(d2g_ctx *ctx, d2g_cmp_set *set, hipStream_t s);
int  d2g_bitslice_sparse_info(d2g_ctx *ctx, const d2g_cmp_set *set, hipStream_t s, uint32_t *out4);
int  d2g_bitslice_sparse_detail(d2g_ctx *ctx, const d2g_cmp_set *set, hipStream_t s, uint64_t *out10);
void d2g_bitslice_fill_detail(const d2g_cmp_set *set, uint64_t *out4);   // host bookkeeping of the last prepare; no synchronisation
SpInit d2g_bitslice_sp_init(const d2g_cmp_set *set);   // what the transpose in front of the set's prepare initialises for its ordering (nothing: a set without sparse state)
int  d2g_bitslice_debug_read(d2g_ctx *ctx, const d2g_cmp_set *set, hipStream_t s, uint64_t *pairs_out, size_t cap, size_t *npairs, uint32_t *root_out);
int  d2g_bitslice_status(d2g_ctx *ctx, const d2g_cmp_set *set, hipStream_t s);   // synchronises; D2G_ERR_INTERNAL on overflow
// exporter set over an N x S_local column slice (no operand of its own); d2g_bitslice_prepare_slice transposes + prepares it
// into the target last given to d2g_bitslice_set_export_target
int  d2g_bitslice_exporter_create(d2g_ctx *ctx, size_t N, size_t S_local, d2g_cmp_set **out);
void d2g_bitslice_set_export_target(d2g_cmp_set *set, uint32_t *planes, uint32_t *meta, uint32_t *status);
int  d2g_bitslice_prepare_slice(d2g_ctx *ctx, d2g_cmp_set *set, const uint64_t *rows_dev, hipStream_t s);
// plane stream of groups [g0, g1) of a gathered operand (the groups before g0 must have their meta in place)
int  d2g_bitslice_derive_groups(d2g_ctx *ctx, const d2g_cmp_set *set, int g0, int g1, hipStream_t s);
// exactly one of (eq_out) or (lut,fout) is non-null
int  d2g_bitslice_ut(d2g_ctx *ctx, const d2g_cmp_set *set, size_t r0, size_t r1, uint32_t *eq_out,
                     const float *lut, float *fout, hipStream_t s);
// multi-GPU engine: the fill of a rank's slab enqueued at the start of the step (under the exchanges)
int  d2g_bitslice_prefill(d2g_ctx *ctx, d2g_cmp_set *set, size_t r0, size_t r1, uint32_t *eq_out, const float *lut, float *fout, hipStream_t s);
// the output of the next upper-triangle launch, announced before the prepare that precedes it: that prepare carries the fill
int  d2g_bitslice_announce(d2g_ctx *ctx, d2g_cmp_set *set, size_t r0, size_t r1, uint32_t *eq_out, const float *lut, float *fout);
void d2g_bitslice_forget(d2g_cmp_set *set);
int  d2g_bitslice_rect(d2g_ctx *ctx, const d2g_cmp_set *set, size_t a0, size_t a1, size_t b0, size_t b1,
                       uint32_t *eq_out, hipStream_t s);

