// d2g_internal.h -- shared between the HIP translation units of libd2g (not installed).
#pragma once
#include "../../include/d2g.h"
#include <hip/hip_runtime.h>
#include <cstdio>
#include <memory>
#include <string>
#include <utility>

#include <vector>
#include "d2g_limits.h"
struct d2g_ctx;
int d2g_hip_status(d2g_ctx *ctx, hipError_t e, const char *what);   // (below) sets last_error to what + ": " + HIP's text; out of memory -> D2G_ERR_NOMEM

// ---- ownership.  The library's structs own GPU resources through the four move-only types below and through nothing else: the
// destructor gives the resource back, so a struct that owns buffers needs no free list.  A plain pointer (or hipStream_t / hipEvent_t)
// field is a VIEW of something another object owns.  Kernels, kernel-argument structs and launches take raw pointers (get() / conversion).
template <class T, bool Pinned> class d2g_owned {
    T *p_ = nullptr; size_t cap_ = 0;
public:
    d2g_owned() = default;
    d2g_owned(d2g_owned &&o) noexcept : p_(o.p_), cap_(o.cap_) { o.p_ = nullptr; o.cap_ = 0; }
    d2g_owned &operator=(d2g_owned &&o) noexcept { if (this != &o) { reset(); p_ = o.p_; cap_ = o.cap_; o.p_ = nullptr; o.cap_ = 0; } return *this; }
    ~d2g_owned() { reset(); }
    void reset() { if (p_) (void)(Pinned ? hipHostFree(p_) : hipFree(p_)); p_ = nullptr; cap_ = 0; }
    // n ELEMENTS in one allocation; `flags` (hipHostMallocDefault, hipHostMallocMapped) applies to pinned memory only
    int alloc(d2g_ctx *ctx, size_t n, const char *what, unsigned flags = hipHostMallocDefault) {
        reset();
        const hipError_t e = Pinned ? hipHostMalloc((void **)&p_, n * sizeof(T), flags) : hipMalloc((void **)&p_, n * sizeof(T));
        if (e != hipSuccess) p_ = nullptr; else cap_ = n;
        return d2g_hip_status(ctx, e, what);
    }
    // grow-only work buffer: the old block is released FIRST (its contents are not kept), then need + need/4 + slack elements are allocated
    int grow(d2g_ctx *ctx, size_t need, size_t slack, const char *what = "work buffer", unsigned flags = hipHostMallocDefault) {
        return need <= cap_ ? D2G_OK : alloc(ctx, need + need / 4 + slack, what, flags);
    }
    T *get() const { return p_; }
    operator T *() const { return p_; }
    size_t cap() const { return cap_; }   // elements
};
template <class T> using d2g_dev = d2g_owned<T, false>;      // one hipMalloc
template <class T> using d2g_pinned = d2g_owned<T, true>;    // one hipHostMalloc

template <class H, hipError_t (*Destroy)(H)> class d2g_handle {
protected:
    H h_ = nullptr;
public:
    d2g_handle() = default;
    d2g_handle(d2g_handle &&o) noexcept : h_(o.h_) { o.h_ = nullptr; }
    d2g_handle &operator=(d2g_handle &&o) noexcept { if (this != &o) { reset(); h_ = o.h_; o.h_ = nullptr; } return *this; }
    ~d2g_handle() { reset(); }
    void reset() { if (h_) (void)Destroy(h_); h_ = nullptr; }
    operator H() const { return h_; }
};
struct d2g_stream : d2g_handle<hipStream_t, hipStreamDestroy> {
    hipError_t create(unsigned flags = hipStreamDefault) { reset(); return hipStreamCreateWithFlags(&h_, flags); }
};
struct d2g_event : d2g_handle<hipEvent_t, hipEventDestroy> {
    hipError_t create(unsigned flags = hipEventDefault) { reset(); return hipEventCreateWithFlags(&h_, flags); }
};

// every timed launch appends a (start, stop) pair; nothing synchronises until the caller asks
struct d2g_evlog {
    std::vector<d2g_event> a, b;
};

// the snapshot of the D2G_* switches (d2g_tuning) and the limits that cut a large call into pieces (d2g_limits_tuning): d2g_limits.h
void d2g_tuning_load(d2g_tuning &t);
// what the switches RESOLVE to (unset or invalid: the default).  The records below are filled once per snapshot of the switches
// (d2g_tuning_resolve, right after d2g_tuning_load) and read as ctx->k2 (K2 kernels and thresholds), ctx->k3_tune (the --multiset
// chain), ctx->limits (d2g_limits.h) and ctx->mgpu_chunks (the multi-GPU engine): nobody parses a switch where it is used.
struct d2g_k2_tuning {
    bool sparse = true;                 // D2G_BS_SPARSE: 0 = every launch walks every tile
    size_t min_n = 8192;                // D2G_BS_SPARSE_MIN_N: below ~6000 sketches the extra launches cost more than the tiles they skip
    int link = 1;                       // D2G_SP_LINK: 0 = no families (every sketch its own segment: the pair list alone; tests)
    double tile_frac = 0.35;            // D2G_SP_TILE_FRAC: the segments may cover this fraction of all tiles before the dense walk is cheaper
    int olink = 1;                      // D2G_SP_OLINK: 0 = the table form of the link passes even where the rank kernel left an owner per value (tests: the multi-GPU engine's form)
    int emit_big = 0;                   // D2G_SP_EMIT_BIG: sp_emit_kernel counts with two words per value at every N (it does from N = 65 536 on; tests)
    int ride = 127;                     // D2G_SP_RIDE: which kernels of the prepare carry an announced output's fill (d2g_cmp_ut_announce_dev) -- 1 column plan (merged schedule: the launch that contains it), 2 flatten (likewise), 4 count, 8 attach, 16 scan, 32 place, 64 the FAST rank kernel's own threads (N <= 12 288; 63 = riders only, as before it); 0 = none, the launch fills (measurements)
    int rank_share = 35;                // D2G_SP_RANK_SHARE: 0 .. 35, the part of an announced fill (in 35ths, like the riders' weights: SP_RW_ALL) the FAST rank kernel writes where bit 64 of D2G_SP_RIDE lets it; at most what its grid holds, six pieces per column (measurements, tests)
    int merge = 2;                      // D2G_K2_MERGE: the prepare's schedule -- 0 = classic, kernel by kernel (column plan and planes in front of the link passes); 1 = merged launches, the planes beside flatten; 2 = merged launches, the planes behind the pair-list kernel's workgroups (d2g_bitslice_prepare; A/B measurements, tests)
    int remember = 1;                   // D2G_SP_REMEMBER: 0 = every prepare runs the ordering, whatever the last one decided
    size_t long_list = 786432;          // D2G_SP_LONG_LIST: a pair list of this many entries or more is binned and composed (the last prepare's length decides)
    int predict = 1;                    // D2G_SP_PREDICT: 0 = no sample before the ordering of a set's first prepare (the ordering finds out by itself, as in round 5)
    int list_form = 0;                  // D2G_SP_LIST_FORM: 1 = always entry by entry, 2 = always binned (tests, measurements)
    size_t list_div = 8;                // D2G_SP_LIST_DIV: the pair list holds at most pairs / list_div entries (and at most 2^27)
    bool sort = true;                   // D2G_BS_SORT: 0 = keep the caller's column order (A/B measurements, tests)
    int tagbits_max = 31;               // D2G_BS_TAGBITS: 0 .. 30 (tests); unset or out of range: 31
    int id16 = 1;                       // D2G_BS_ID16: 0 = 32-bit column ids in every set (1: 16-bit ids where the rank kernel is single-partition, N <= 21 845; A/B measurements, tests)
    int nsplit_req = 0;                 // D2G_BS_NSPLIT: 1, 2 or 4 rank workgroups per column where the hash space has that many partitions (tests / experiments); 0 = automatic
};
d2g_k2_tuning d2g_k2_tuning_resolve(const d2g_tuning &t);   // (d2g_runtime.hip)
std::string d2g_k2_tuning_json(const d2g_ctx *ctx);   // (d2g_k2_bitslice.hip) {"D2G_BS_SPARSE_MIN_N": 8192, ...}: the resolved values of the same switches
uint64_t d2g_k2_tuning_hash(const d2g_ctx *ctx);   // (d2g_k2_bitslice.hip) FNV-1a over the RESOLVED values of the switches that select K2 kernels and thresholds: what the ranks of one job must agree on

// K3's bucket geometry (d2g_k3_bucket.hip, d2g_k3_bmh.hip), here because the defaults and limits of its switches are these constants
constexpr int K3_MAXBBITS = 12;             // log2 of the most buckets per genome (LDS histogram)
constexpr int K3_ROUND_KEYS = 1400;         // keys one table round is sized for (load <= 0.69 of the 2048-slot LDS count table)
constexpr int K3_TARGET = 1024;             // mean keys per bucket aimed for
constexpr int K3_L1BITS = 8;                // write fronts of the scatter = 2^K3_L1BITS; the other bucket bits are resolved by k3_refine_kernel
constexpr uint64_t K3_SPLIT_MIN = 4 * 1400; // mean bucket size above which a genome's buckets are split once more
struct d2g_k3_tuning {
    bool compact = false;               // D2G_K3_COMPACT: 1 = 4-byte stored words and the tile-sorted split, where k allows it (k <= 21: decided per call)
    bool light = true;                  // D2G_K3_LIGHT: 0 = the first pass in the heavy form too (no survivor queue in HBM)
    uint32_t l1bits = K3_L1BITS;        // D2G_K3_L1BITS: 0 .. K3_MAXBBITS bucket bits the scatter resolves itself; the rest is k3_refine_kernel's
    uint64_t bucket_keys = K3_TARGET;   // D2G_K3_BUCKET_KEYS: mean keys per bucket the generic path aims for (tests: small inputs with many buckets)
    uint64_t sub_keys = K3_TARGET;      // D2G_K3_SUB_KEYS: mean keys per sub-range when a big genome's buckets are split once more
    uint64_t split_min = 0;             // D2G_K3_SPLIT_MIN: buckets averaging more keys than this are split once more; 0 = automatic (by path: K3_ROUND_KEYS compact, K3_SPLIT_MIN generic)
    size_t subbatch = 0;                // D2G_K3_SUBBATCH: 1 .. 8 genome ranges of the bucketing / counting pipeline; 0 = automatic (4 for >= 8 genomes and >= 2e8 k-mers, else 1)
    uint32_t round_keys = K3_ROUND_KEYS;// D2G_K3_ROUND_KEYS: 1 .. K3_ROUND_KEYS keys per table round (tests force multi-round buckets on small inputs)
    double guess_scale = 1.0;           // D2G_K3_GUESS_SCALE: factor on the first guess of the BagMinHash bound, genomes and explicit weighted sets alike (tests force the redo passes)
    size_t grid_per_cu = 48;            // D2G_K3_GRID_PER_CU: 1 .. 256 workgroups of the main pass per CU
    bool gq_scale_set = false;          // D2G_K3_GQ_SCALE was given (tests force the region overflow) ...
    double gq_scale = 2.0;              // ... a survivor region holds this multiple of the survivors expected in it ...
    uint64_t gq_slack = 256;            // ... plus this many entries: 1 when the scale was given, else 256 above 24 workgroups per CU and 1024 up to there
    uint64_t sort_keys = K3_TARGET;     // D2G_K3S_RANGE_KEYS: 1 .. K3_TARGET mean keys per sort range of the sorted emission, K3s (tests: small inputs with many ranges)
    uint64_t cs_table_bytes = 0;        // D2G_CS_TABLE_BYTES: the count-sketch table (K3k) takes at most this many bytes, so a batch goes in more groups of genomes (debugging, tests); 0 = a sixth of the free device memory
    int cs_lds_cells = -1;              // D2G_CS_LDS_CELLS: 0 .. 40960, the most cells K3k accumulates in LDS (0: every table in global memory; measurements); -1 = K3K_LDS_CELLS
};
// the exact-set compare (d2g_kset_cmp.hip)
struct d2g_kset_tuning {
    int split = 0;                      // D2G_KSET_SPLIT: workgroups a tile's slice range is cut across: 1 = the one-workgroup route (plain stores), >= 2 = the atomic route with that many; 0 = automatic
    int pbits = -1;                     // D2G_KSET_PBITS: 0 .. 20 key bits that cut the key space into slices (tests); -1 = from the largest set
};
// the edit-distance kernel (d2g_edit.hip)
struct d2g_edit_tuning {
    int strip = 0;                      // D2G_EDIT_STRIP: 1 .. 64, at most this many 32-row blocks of a query per strip (tests: the several-strip route on short records); 0 = what LDS holds
    int tile = 0;                       // D2G_EDIT_TILE: 1 .. 65536 column records per workgroup (tests, measurements); 0 = by launch class (512, 64, 8)
    int dedup_route = 0;                // D2G_EDIT_DEDUP_ROUTE: 1 = the list kernel wherever it exists, 2 = the all-columns route for every row (measurements, tests: d2g_edit_dedup.hip); 0 = the dispatcher's choice
    int dedup_reverse = 0;              // D2G_EDIT_DEDUP_REVERSE: 1 = the representative list is written backwards (tests: the result does not depend on its order)
    int near_route = 0;                 // D2G_EDIT_NEAR_ROUTE: 1 = the band route wherever it exists, 2 = the full route everywhere (measurements: the crossover of d2g_edit_near.hip); 0 = the dispatcher's choice
};
d2g_k3_tuning d2g_k3_tuning_resolve(const d2g_tuning &t);   // (d2g_runtime.hip)
constexpr int MG_MAX_CHUNKS = 4;            // most chunks a rank's column slice is cut into inside one multi-GPU step (d2g_mgpu.hip)
void d2g_tuning_resolve(d2g_ctx *ctx);      // (d2g_runtime.hip) d2g_tuning_load, then every record above

struct d2g_ctx {
    int device = -1;
    d2g_tuning tune;
    d2g_k2_tuning k2;                       // ... and what its K2 switches resolved to,
    d2g_k3_tuning k3_tune;                  // its K3 switches,
    d2g_kset_tuning kset;                   // the exact-set compare's,
    d2g_edit_tuning edit;                   // the edit-distance kernel's,
    d2g_limits_tuning limits;               // the limits that cut a large call into pieces (tests shrink them: d2g_limits.h),
    int mgpu_chunks = 0;                    // and D2G_MGPU_CHUNKS: 1 .. MG_MAX_CHUNKS; 0 = the engine's default (a function of the shape)
    int num_cus = 0;
    std::string last_error;
    int timing = 0;                         // D2G_TIME_* mask (d2g_set_timing)
    d2g_evlog ev_k1, ev_k2, ev_k2prep, ev_k3, ev_k0, ev_knn;
    d2g_evlog ev_k1count;                   // "k1count": the count pass after K1 (d2g_oph_count_dev), timed under D2G_TIME_K1
    d2g_evlog ev_k1i, ev_k1iexpand, ev_k1ibmh;   // interval inputs (d2g_k1i.hip): "k1i" = the OPH kernel, under D2G_TIME_K1; under D2G_TIME_K3 "k1iexpand" = runs -> (id, weight) lists, "k1ibmh" = BagMinHash over them
    d2g_evlog ev_filter;                    // "filter": the build of a k-mer filter's table (d2g_kmer_filter_create_dev), under D2G_TIME_FILTER
    d2g_evlog ev_k3k, ev_k3kcompact, ev_k3kbmh;   // under D2G_TIME_K3, the count-sketch chain (K3k): "k3k" = zeroing and k3k_add_kernel, "k3kcompact" = table -> (cell, |count|) lists, "k3kbmh" = BagMinHash over them
    d2g_evlog ev_k3s, ev_kset, ev_ksetprep; // under D2G_TIME_KSET: "k3s" = the sorted emission after K3's count (d2g_kmer_sets*), "kset" = the exact pair kernel, "ksetprep" = a d2g_kset's slice table
    d2g_evlog ev_edit, ev_editprep;         // under D2G_TIME_EDIT (d2g_edit.hip): "edit" = the pair kernel's launches of one call, "editprep" = a d2g_seqset's upload and recoding
    d2g_evlog ev_editnear;                  // under D2G_TIME_EDIT_NEAR (d2g_edit_near.hip): "editnear" = the band kernel's and the clamp kernel's launches of one call (the full route's pair kernel is logged as "edit")
    d2g_evlog ev_editdedup, ev_editdedup_list, ev_editdedup_resolve;   // under D2G_TIME_EDIT_DEDUP (d2g_edit_dedup.hip): "editdedup" = every kernel of one band of d2g_edit_dedup_dev; inside it "editdedup_list" = the two kernels that compact the representative list, "editdedup_resolve" = the in-order step
    d2g_evlog ev_screen, ev_screenreduce, ev_screenbuild;   // under D2G_TIME_SCREEN (d2g_screen.hip): "screen" = the count walk, "screenreduce" = d2g_screen_result's kernel, "screenbuild" = a screen's table
    d2g_evlog ev_dedup, ev_dedup_resolve;   // "dedup" = both: the per-row kernel and the in-order step of d2g_cmp_dedup_dev ("dedup_resolve": the latter alone)
    struct d2g_k3_state *k3 = nullptr;      // work buffers of d2g_bmh_sketch_dev (d2g_k3.h)
    uint64_t cs_table_bytes = 0, cs_groups = 0, cs_batches = 0;   // K3k (d2g_countsketch_stats): the largest table so far, the groups and the batches of all count-sketch calls
    d2g_dev<uint32_t> knn_band;             // [band rows][N] equality counts the selection kernel reads (d2g_knn.hip); grow-only
    d2g_dev<unsigned long long> dedup_keys; // one key per row of a band: its best representative of earlier bands (d2g_dedup.hip, d2g_edit_dedup.hip)
    d2g_dev<uint32_t> edit_dedup_ws;        // d2g_edit_dedup.hip: the representative list [N], its length, the compaction's counts, the band's own block; grow-only
};
void d2g_k3_state_destroy(struct d2g_k3_state *st);
// (d2g_knn.hip) the selection kernel of K2e over rows [row0, row0 + nrows) of a band [nrows][N] of values in [0, S] that the caller filled
int d2g_knn_select_band(d2g_ctx *ctx, const uint32_t *band, size_t N, size_t S, size_t K, uint32_t min_count, size_t row0, size_t nrows, size_t out0,
                        size_t cap, uint32_t *rowcnt_dev, uint32_t *ids_dev, uint32_t *counts_dev, hipStream_t s);
// (d2g_host.cpp) the host ranking behind d2g_screen_create: distinct keys ascending, their raw k-mers, the rank of every position's key
void d2g_screen_rank_keys(const uint64_t *keys, size_t n, uint64_t xormask, std::vector<uint64_t> &distinct, std::vector<uint64_t> &raw,
                          std::vector<uint32_t> &rank);
// (d2g_k3_lists.hip) BagMinHash (BMH-D2G) over (id, weight) lists that lie in device memory: set i = elements [set_off[i], set_off[i + 1])
// of ids_dev / w_dev, set_off and the total weights tw host arrays [ng + 1] / [ng]; registers to the host array sig_out [ng][m].  Every
// weight must be > 0 and <= 2^53.  Enqueues on `s` and waits for it; `ev` times the walk (under D2G_TIME_K3).
int d2g_bmh_device_lists(d2g_ctx *ctx, hipStream_t s, const uint64_t *ids_dev, const double *w_dev, const uint64_t *set_off, const double *tw,
                         size_t ng, size_t m, double *sig_out, d2g_evlog *ev);
inline int d2g_hip_status(d2g_ctx *ctx, hipError_t e, const char *what) {
    if (e == hipSuccess) return D2G_OK;
    ctx->last_error = std::string(what) + ": " + hipGetErrorString(e);
    return e == hipErrorOutOfMemory ? D2G_ERR_NOMEM : D2G_ERR_HIP;
}

#define D2G_HIP(ctx, call)                                                            \
    do {                                                                              \
        hipError_t e__ = (call);                                                      \
        if (e__ != hipSuccess) {                                                      \
            (ctx)->last_error = std::string(#call) + ": " + hipGetErrorString(e__);   \
            return e__ == hipErrorOutOfMemory ? D2G_ERR_NOMEM : D2G_ERR_HIP;          \
        }                                                                             \
    } while (0)

#define D2G_CHECK(ctx, cond, msg)                      \
    do {                                               \
        if (!(cond)) {                                 \
            (ctx)->last_error = (msg);                 \
            return D2G_ERR_INVALID;                    \
        }                                              \
    } while (0)

// hipEvent bracket around the dominant kernel of a path (enabled with d2g_set_timing);
// elapsed times are read lazily by d2g_kernel_ms (which synchronises on the stop events).
struct d2g_timer {
    d2g_evlog *ev; hipStream_t s; bool on;
    d2g_timer(d2g_ctx *c, d2g_evlog *e, hipStream_t st) : ev(e), s(st), on(false) {
        const int bit = (e == &c->ev_k1 || e == &c->ev_k1count || e == &c->ev_k1i) ? D2G_TIME_K1 : e == &c->ev_k2 ? D2G_TIME_K2 : e == &c->ev_k2prep ? D2G_TIME_K2PREP : e == &c->ev_k0 ? D2G_TIME_K0 : e == &c->ev_knn ? D2G_TIME_KNN : e == &c->ev_filter ? D2G_TIME_FILTER : (e == &c->ev_k3s || e == &c->ev_kset || e == &c->ev_ksetprep) ? D2G_TIME_KSET : (e == &c->ev_dedup || e == &c->ev_dedup_resolve) ? D2G_TIME_DEDUP : (e == &c->ev_edit || e == &c->ev_editprep) ? D2G_TIME_EDIT : e == &c->ev_editnear ? D2G_TIME_EDIT_NEAR : (e == &c->ev_editdedup || e == &c->ev_editdedup_list || e == &c->ev_editdedup_resolve) ? D2G_TIME_EDIT_DEDUP : (e == &c->ev_screen || e == &c->ev_screenreduce || e == &c->ev_screenbuild) ? D2G_TIME_SCREEN : D2G_TIME_K3;
        on = (c->timing & bit) != 0;
        if (on) {
            d2g_event x, y;
            if (x.create() != hipSuccess || y.create() != hipSuccess) { on = false; return; }
            (void)hipEventRecord(x, s);
            ev->a.push_back(std::move(x)); ev->b.push_back(std::move(y));
        }
    }
    void stop() { if (on) (void)hipEventRecord(ev->b.back(), s); }
};

// one per translation unit with kernels: makes the runtime load that unit's code object now (hipFuncGetAttributes on one of
// its kernels) instead of at its first launch
void d2g_warm_filter(); void d2g_warm_k0(); void d2g_warm_k1(); void d2g_warm_k1i(); void d2g_warm_k2(); void d2g_warm_k2_bitslice(); void d2g_warm_k2_planes(); void d2g_warm_k3(); void d2g_warm_kset(); void d2g_warm_screen(); void d2g_warm_knn(); void d2g_warm_dedup(); void d2g_warm_edit(); void d2g_warm_edit_near(); void d2g_warm_edit_dedup();

static inline hipStream_t as_stream(void *s) { return reinterpret_cast<hipStream_t>(s); }

template <class T> static inline T div_up(T a, T b) { return (a + b - 1) / b; }
