/*
 * d2g.h -- C ABI of libd2g.so: the MI355X (gfx950) implementation of dashing2's two
 * data-parallel hot paths.  This is the drop-in boundary: plain pointers and sizes,
 * no C++ / torch types, no exceptions across the ABI.
 *
 * dashing2 has no FFI of its own; the seams this library replaces are the C++ calls
 *   fastx2sketch()      reference src/fastxsketch.h:66   (called at sketch_core.cpp:31)
 *   cmp_core()/compare()/emit_rectangular()   reference src/cmp_main.h:130-132
 * INTEGRATION.md shows the few lines a dashing2 maintainer would add at those seams.
 *
 * Conventions
 *   - every call returns 0 on success or a negative d2g_status; d2g_strerror() names it and
 *     d2g_last_error(ctx) carries the HIP/runtime detail.
 *   - `_dev` entry points take DEVICE pointers (caller-owned, e.g. from d2g_malloc or a
 *     torch tensor's data_ptr) and a hipStream_t passed as void* (NULL = default stream);
 *     they enqueue work and do not synchronise.  Entry points without `_dev` take HOST
 *     pointers, move the data, run, synchronise and copy results back.
 *   - a d2g_ctx is bound to one GPU and is used by one host thread at a time
 *     (multi-GPU = one process / one ctx per device).
 *   - there is NO CPU fallback: without a usable gfx950 device d2g_ctx_create fails.
 */
#ifndef D2G_H
#define D2G_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define D2G_VERSION_MAJOR 0
#define D2G_VERSION_MINOR 1

typedef struct d2g_ctx d2g_ctx;

enum d2g_status {
    D2G_OK = 0,
    D2G_ERR_INVALID = -1,      /* bad argument (the reference would throw std::invalid_argument) */
    D2G_ERR_NODEVICE = -2,     /* no usable HIP device */
    D2G_ERR_HIP = -3,          /* HIP runtime error; see d2g_last_error */
    D2G_ERR_NOMEM = -4,
    D2G_ERR_UNSUPPORTED = -5,  /* outside the hot-path scope (e.g. k > 32) */
    D2G_ERR_IO = -6,
    D2G_ERR_INTERNAL = -7      /* an internal invariant failed (reported, never silent) */
};

/* measures: order of enum Measure, reference src/cmp_main.h:8-17 */
enum d2g_measure {
    D2G_SIMILARITY = 0, D2G_CONTAINMENT = 1, D2G_SYMMETRIC_CONTAINMENT = 2,
    D2G_POISSON_LLR = 3, D2G_INTERSECTION = 4, D2G_UNION_SIZE = 5
};

/* which all-pairs kernel family to use (d2g_cmp_* `algo` argument) */
enum d2g_cmp_algo {
    D2G_CMP_AUTO = 0,       /* bit-sliced when it applies, else direct */
    D2G_CMP_DIRECT = 1,     /* 64-bit register compare, LDS-tiled */
    D2G_CMP_BITSLICE = 2,   /* per-column dense ids -> bit planes -> v_bitop3/v_bcnt */
    D2G_CMP_PLANES = 3      /* sets of truncated codes (d2g_cmp_set_create_codes): bit planes of the codes, bit-serial order compare */
};

/* ---- runtime ------------------------------------------------------------ */
int         d2g_version(void);                       /* major*1000 + minor */
const char *d2g_strerror(int status);
int         d2g_device_count(void);
int         d2g_ctx_create(int device, d2g_ctx **out);
void        d2g_ctx_destroy(d2g_ctx *ctx);
const char *d2g_last_error(const d2g_ctx *ctx);
int         d2g_ctx_device(const d2g_ctx *ctx);
/* The library's D2G_* tuning switches and test hooks are read from the environment ONCE, when the context is
 * created; d2g_ctx_reload_tuning reads them again (tests that change a switch between calls).  d2g_ctx_tuning writes the resolved
 * set as a JSON object {"D2G_X": "value", ...} (only the switches that were set) into buf and returns the length it needs. */
int         d2g_ctx_reload_tuning(d2g_ctx *ctx);
int         d2g_ctx_tuning(const d2g_ctx *ctx, char *buf, size_t cap);
int         d2g_sync(d2g_ctx *ctx, void *stream);
int         d2g_malloc(d2g_ctx *ctx, size_t nbytes, void **dptr);
int         d2g_free(d2g_ctx *ctx, void *dptr);
/* device memory free now and in all, in bytes (a caller that sizes a resident object, e.g. the rows of a d2g_screen) */
int         d2g_mem_info(d2g_ctx *ctx, size_t *free_bytes, size_t *total_bytes);
/* page-locked host memory: D2H/H2D at PCIe rate, no per-batch page faults */
int         d2g_malloc_host(d2g_ctx *ctx, size_t nbytes, void **hptr);
int         d2g_free_host(d2g_ctx *ctx, void *hptr);
/* page-lock / release memory the caller owns (an ingest pipeline can start filling its staging buffers before the context
 * exists and register them once it does) */
int         d2g_host_register(d2g_ctx *ctx, void *hptr, size_t nbytes);
int         d2g_host_unregister(d2g_ctx *ctx, void *hptr);
/* Pays one-time costs NOW -- on whatever thread calls it, e.g. a helper thread that has just created the context while the main
 * thread is still reading its inputs -- instead of inside the first real operation: D2G_WARM_COPY = the runtime's copy machinery
 * (the first host<->device copy of a process costs ~30 ms, whatever its size), D2G_WARM_K* = the code objects of a kernel family
 * (D2G_WARM_K1 and D2G_WARM_K3 include the filtered instantiations of their k-mer walkers and the filter's own kernels). */
#define D2G_WARM_COPY 1
#define D2G_WARM_K0   2
#define D2G_WARM_K1   4
#define D2G_WARM_K2   8
#define D2G_WARM_K3   16
#define D2G_WARM_KSET 32
#define D2G_WARM_SCREEN 64
#define D2G_WARM_K1I  128     /* the interval kernels (K1i, below) */
#define D2G_WARM_EDIT 256     /* the edit-distance kernels (K2h, below) */
int         d2g_warmup(d2g_ctx *ctx, int what);
/* "<marketing name> (<gcn arch>, <n> CUs)" of a device, for logs and --gpu-stats */
int         d2g_device_name(int device, char *buf, size_t cap);
int         d2g_memcpy_h2d(d2g_ctx *ctx, void *dst_dev, const void *src_host, size_t nbytes, void *stream);
int         d2g_memcpy_d2h(d2g_ctx *ctx, void *dst_host, const void *src_dev, size_t nbytes, void *stream);
/* Per-launch HIP-event timing of the dominant kernels.  With timing enabled every launch of
 * the K1 kernel ("k1"), its count pass ("k1count", also under D2G_TIME_K1), the interval kernel ("k1i", likewise; "k1iexpand" and "k1ibmh" under D2G_TIME_K3), the K0 ingest chain ("k0"), the build of a k-mer filter ("filter"), the K3 chain ("k3"), the K2 pair kernel ("k2") and the K2 prepare chain ("k2prep") is
 * bracketed by events recorded on the launch stream; nothing synchronises until d2g_kernel_ms,
 * which reports the number of logged launches, their average and the last duration (ms) and
 * optionally clears the log. */
#define D2G_TIME_K1     2
#define D2G_TIME_K2     4
#define D2G_TIME_K2PREP 8
#define D2G_TIME_K3     16
#define D2G_TIME_K0     32
#define D2G_TIME_KNN    64      /* "knn": the selection kernel of d2g_cmp_knn_dev (its count walk is logged as "k2") */
#define D2G_TIME_DEDUP  128     /* "dedup": the per-row kernel and the in-order step of d2g_cmp_dedup_dev ("dedup_resolve": the in-order
                                 * step alone; the count walk is logged as "k2") */
#define D2G_TIME_FILTER 256     /* "filter": the build of a k-mer filter's table (d2g_kmer_filter_create*) */
#define D2G_TIME_KSET   512     /* "k3s": the sorted emission of d2g_kmer_sets* (behind the count chain, which is logged as "k3"); "kset": the exact
                                 * pair kernel of d2g_kset_isz_*_dev; "ksetprep": the slice table of a d2g_kset */
#define D2G_TIME_SCREEN 1024    /* "screen": the count walk of d2g_screen_add_dev / d2g_sketcher_run_screen; "screenreduce": the per-reference
                                 * sums of d2g_screen_result; "screenbuild": the table of d2g_screen_create */
#define D2G_TIME_EDIT   2048    /* "edit": the pair kernel of d2g_edit_*_dev (the launches of one call under one bracket); "editprep": the upload and
                                 * recoding of d2g_seqset_create */
#define D2G_TIME_EDIT_NEAR 4096 /* "editnear": the band kernel and the clamp kernel of d2g_edit_near_dev (K2i), one bracket per run of consecutive
                                 * rows that take one route (a call whose rows all take one route: one bracket; sum count x avg for a mixed
                                 * call); the pair kernel of its full route is logged as "edit", the selection of d2g_edit_within_dev as "knn" */
#define D2G_TIME_EDIT_DEDUP 8192 /* "editdedup": the kernels of d2g_edit_dedup_dev (K2j) under one bracket per band; inside it "editdedup_list" = the
                                 * two kernels that compact the representative list, "editdedup_resolve" = the in-order step; the kernels of
                                 * d2g_edit_near_dev for rows on the all-columns route are also logged under their own names */
/* enabled: 0 = off, 1 = every kernel above, or an OR of D2G_TIME_* (an event pair in the stream costs a few microseconds of
 * device time per launch: time only what is being reported) */
int         d2g_set_timing(d2g_ctx *ctx, int enabled);
int         d2g_kernel_ms(d2g_ctx *ctx, const char *which, int reset, int *count, float *avg_ms, float *last_ms);

/* ---- host-side primitives of the path (x86, x87 long double where the reference uses it) ---- */
/* sketch::hash::WangHash::hash -- reference call sites src/enums.h:136-140, src/oph.h:44-53 */
uint64_t d2g_wang_hash(uint64_t x);
/* seed_mask(): reference src/enums.cpp:131-140.  0 -> 0 (CLI default, sketch_main.cpp:112) */
uint64_t d2g_seed_mask(uint64_t seedseed);
/* DHasher xor constant seed_ ^ 0x533f8c2151b20f97: reference src/oph.h:44-53,59,142 */
uint64_t d2g_oph_xor_const(void);
/* sketch::hash::WangHash::inverse: d2g_wang_hash_inverse(d2g_wang_hash(x)) == x for every x */
uint64_t d2g_wang_hash_inverse(uint64_t x);
/* LazyOnePermSetSketch ctor: m = S rounded up to even. reference src/oph.h:143-146 */
size_t   d2g_oph_m(size_t sketchsize);
/* ids(): the masked k-mer behind every register, DHasher::inverse (reference src/oph.h:50-52,81-83,162-164,264-271):
 * ids_out[i][r] = d2g_oph_xor_const() ^ d2g_wang_hash_inverse(regs[i][r]) for r < S, the first S of every m (reference
 * src/fastxsketch.cpp:619-620).  This is maskfn(kmer) = d2g_wang_hash(kmer ^ xormask), which the reference's invmaskfn turns back
 * into bases.  An empty register (~0) decodes like any other value. */
int      d2g_oph_kmer_ids(const uint64_t *regs /* [n][m] */, size_t n, size_t m, size_t sketchsize, uint64_t *ids_out /* [n][S] */);
/* getcard(): reference src/oph.h:240-247 */
double   d2g_oph_card(const uint64_t *regs, size_t m);
/* data(): u64 registers -> double signatures. reference src/oph.h:248-263 */
int      d2g_oph_signatures(const uint64_t *regs, size_t m, double *sig_out /* [m] */);
/* both, for n sketches; writes the first S of each m (reference src/fastxsketch.cpp:605,610) */
int      d2g_oph_finalize(const uint64_t *regs /* [n][m] */, size_t n, size_t m, size_t sketchsize,
                          double *sigs_out /* [n][S] */, double *cards_out /* [n] */, int nthreads);
/* densify(): reference src/cmp_core.cpp:577-613 (caller 686-718). In place. Returns #filled via *nfilled. */
int      d2g_densify(double *sigs /* [n][S] */, size_t n, size_t sketchsize, size_t *nfilled, int nthreads);
/* compare() epilogues: reference src/cmp_core.cpp:458-494 (set space, from gt/lt) and
 * 495-517 (multiset space, from neq), both followed by 573-575. */
float    d2g_epilogue_gtlt(uint64_t gt, uint64_t lt, size_t sketchsize, double lhcard, double rhcard,
                           int measure, int k);
float    d2g_epilogue_neq(uint64_t neq, size_t sketchsize, double lhcard, double rhcard, int measure, int k);
/* the same epilogues over rows [r0,r1) of the condensed upper triangle from the device's integer
 * counts (OpenMP): ca = neq, or gt when cb (= lt) is non-null.  With cb == NULL in set space the
 * sketch size must be a power of two (then only gt+lt = S-neq matters: every multiple of 1/S is exact). */
int      d2g_epilogue_ut(const uint32_t *ca, const uint32_t *cb, const double *cards, size_t N, size_t sketchsize,
                         size_t r0, size_t r1, int measure, int k, int multiset_space, int nthreads, float *out);
/* table t[neq] = epilogue for card-independent measures (SIMILARITY, POISSON_LLR) when the
 * value depends on neq only (power-of-two S in set space; any S in multiset space).
 * Returns D2G_ERR_UNSUPPORTED otherwise. lut_out has S+1 floats. */
int      d2g_epilogue_lut(size_t sketchsize, int measure, int k, int multiset_space, float *lut_out);

/* ---- truncated registers: the reference's --fastcmp <4|2|1> (alias --regsize, --regbytes) and --bbit-sigs --------
 * make_compressed(), reference src/cmp_core.cpp:209-322: the n x S matrix of (densified) double signatures becomes
 * codes of regbytes in {1, 2, 4} (codes_out: uint8/uint16/uint32 [n][S]).
 *   bbit == 0, "setsketch" (:246-292): minreg/maxreg over the registers that are > 0 and != DBL_MAX, q = 254.3 / 65534 /
 *     4294967294, b = expl(logl(max/min)/q), a = max/b (CSetSketch::optimal_parameters, src/setsketch.cpp:7-10),
 *     code = max(0, min(int64(q + 1), (int64)(1.L - logl(sig/a) / log1pl(b - 1.L)))) in x87 long double.  A register <= 0
 *     makes that cast undefined in C++; its code is DEFINED here as 0, which is what the reference's x86 build yields
 *     (the conversion gives the "integer indefinite" INT64_MIN, and the clamp then 0).  ab_out[0] = a, ab_out[1] = b;
 *     minmax_out (may be NULL) = {minreg, maxreg}.
 *   bbit != 0 (:294-320): code = WangHash(bits(sig) ^ 0xa3407fb23cd20ef) >> (58 | 48 | 32): a byte code has SIX significant
 *     bits -- the reference's shift table, kept.  ab_out = {0, 0}.
 * Returns D2G_ERR_INVALID with a message in err (may be NULL) for: regbytes not in {1, 2, 4}; a matrix without any finite
 * positive register; a register that is +inf; a or b zero, infinite or NaN (the reference falls back to b-bit codes there but
 * keeps the (gt, lt) epilogue with b = 0 -- not reproduced, SURVEY's list of reference defects). */
int      d2g_regs_truncate(const double *sigs /* [n][S] */, size_t n, size_t sketchsize, int regbytes, int bbit, void *codes_out,
                           long double *ab_out /* [2] */, double *minmax_out /* [2] or NULL */, int nthreads, char *err, size_t errcap);
/* the compressed branch of compare(), reference src/cmp_core.cpp:362-449, followed by 573-575 and the conversion to float:
 * from the number of equal b-bit codes (:406-423; fmal(neq, 1.L/S, -2^-(8 regbytes)) is ONE rounding) ... */
float    d2g_epilogue_trunc_neq(uint64_t neq, size_t sketchsize, int regbytes, double lhcard, double rhcard, int measure, int k);
/* ... and from (#a>b, #a<b) of setsketch codes and their base *b (:425-448, g_b :323-325).  The sketch space plays no part. */
float    d2g_epilogue_trunc_gtlt(uint64_t gt, uint64_t lt, size_t sketchsize, const long double *b, double lhcard, double rhcard,
                                 int measure, int k);
/* array forms (OpenMP) over rows [r0,r1) of the condensed upper triangle and over the row-major block rows [a0,a1) x columns
 * [b0,b1), compare(row, column).  b == NULL: ca = neq of b-bit codes (cb unused); otherwise ca = gt, cb = lt, and g_b(b, c/S)
 * is tabulated once for its S+1 arguments (no powl per pair). */
int      d2g_epilogue_trunc_ut(const uint32_t *ca, const uint32_t *cb, const double *cards, size_t N, size_t sketchsize,
                               size_t r0, size_t r1, int measure, int k, int regbytes, const long double *b, int nthreads, float *out);
int      d2g_epilogue_trunc_rect(const uint32_t *ca, const uint32_t *cb, const double *cards, size_t N, size_t sketchsize,
                                 size_t a0, size_t a1, size_t b0, size_t b1, int measure, int k, int regbytes,
                                 const long double *b, int nthreads, float *out);

/* ---- host ingest: FASTA/FASTQ(.gz) -> packed run stream (input of K1) -------------
 * Replaces the parsing half of bns::Encoder::for_each + kseq (reference call sites
 * src/fastxsketch.cpp:383-424 ; src/d2.h:52-71 for_each_substr ; src/d2.h:273-305 KSeqHolder).
 * One "genome" = one input line of the reference (a path, or several space-separated paths
 * that feed the same sketch).  Records and non-ACGT bytes end a run; runs shorter than k
 * are dropped (they contain no k-mer). */
typedef struct d2g_seqpack d2g_seqpack;
int  d2g_seqpack_create(int k, d2g_seqpack **out);
/* the same under an alphabet (K1a below): D2G_ALPHABET_DNA is d2g_seqpack_create; under a protein alphabet the stream holds ONE BYTE
 * per residue (its code), the runs are the maximal runs of the alphabet's letters, and every add_* form works as it does for DNA.
 * k above d2g_alphabet_max_k or an unknown alphabet is D2G_ERR_UNSUPPORTED. */
int  d2g_seqpack_create_alphabet(int k, int alphabet, d2g_seqpack **out);
int  d2g_seqpack_alphabet(const d2g_seqpack *sp);
void d2g_seqpack_destroy(d2g_seqpack *sp);
/* forget the content but keep the allocations (pooling packers avoids page-fault storms) */
void d2g_seqpack_clear(d2g_seqpack *sp);
/* appends one genome from a file "line" (gz transparently via zlib). */
int  d2g_seqpack_add_path(d2g_seqpack *sp, const char *path_line);
/* appends one genome from ONE file whose name is taken as it stands, spaces included (gz transparently) */
int  d2g_seqpack_add_file(d2g_seqpack *sp, const char *path);
/* appends one genome from an in-memory FASTA/FASTQ buffer */
int  d2g_seqpack_add_fastx(d2g_seqpack *sp, const char *buf, size_t len);
/* appends one genome consisting of a single raw sequence (no header) */
int  d2g_seqpack_add_sequence(d2g_seqpack *sp, const char *seq, size_t len);
/* --parse-by-seq (reference src/fastxsketchbyseq.cpp:233-252): every FASTA/FASTQ record of the file(s)
 * becomes its own genome, named by its header up to the first whitespace (kseq's name); records
 * without a k-mer still get an (empty) genome so that indices line up with the reference's names_. */
int             d2g_seqpack_add_path_by_record(d2g_seqpack *sp, const char *path_line);
int             d2g_seqpack_add_fastx_by_record(d2g_seqpack *sp, const char *buf, size_t len);
const char     *d2g_seqpack_name(const d2g_seqpack *sp, size_t genome);   /* packs filled by *_by_record only */
size_t          d2g_seqpack_ngenomes(const d2g_seqpack *sp);
size_t          d2g_seqpack_nruns(const d2g_seqpack *sp);
size_t          d2g_seqpack_packed_bytes(const d2g_seqpack *sp);   /* including the 64-byte pad */
const uint8_t  *d2g_seqpack_packed(const d2g_seqpack *sp);
const uint64_t *d2g_seqpack_run_start(const d2g_seqpack *sp);
const uint32_t *d2g_seqpack_run_len(const d2g_seqpack *sp);
const uint64_t *d2g_seqpack_genome_run_off(const d2g_seqpack *sp);  /* [ngenomes+1] */
uint64_t        d2g_seqpack_nkmers(const d2g_seqpack *sp, size_t genome); /* = total_updates */
uint64_t        d2g_seqpack_nbases(const d2g_seqpack *sp);           /* bases stored */

/* ---- K1: 2-bit packed bases -> OPH registers ---------------------------------
 * Replaces the per-k-mer chain bns::Encoder::for_each -> maskfn -> OPSetSketch::update
 * (reference src/fastxsketch.cpp:383-424,565 ; src/enums.h:136-140 ; src/oph.h:176-211).
 *
 * Input layout ("packed run stream"):
 *   packed      2 bits per base, A0 C1 G2 T3, base p at bits [2(p%4), 2(p%4)+2) of byte p/4.
 *               Only the maximal ACGT runs of length >= k are stored, back to back; the
 *               buffer must be padded with >= 64 readable bytes after the last base.
 *   run_start   [nrun]   first base (index into the packed stream) of each run
 *   run_len     [nrun]   run length in bases (>= k)
 *   genome_run_off [n+1] runs of genome g are [genome_run_off[g], genome_run_off[g+1])
 * k-mers never span runs (window resets at non-ACGT bytes and record boundaries).
 * Output: regs_out[n][m] (m = d2g_oph_m(S)), each register = min OPH id of its bucket or ~0.
 * This and the other host-pointer one-shots (d2g_oph_sketch_counts, d2g_kmer_filter_create, d2g_bmh_sketch, d2g_kmer_count,
 * d2g_kmer_distinct) are the d2g_sketcher form of the call on a sketcher that lives for that call: convenient, not for loops.
 */
int d2g_oph_sketch(d2g_ctx *ctx, const uint8_t *packed, size_t packed_bytes,
                   const uint64_t *run_start, const uint32_t *run_len, size_t nrun,
                   const uint64_t *genome_run_off, size_t n,
                   int k, int canon, uint64_t xormask, size_t sketchsize,
                   uint64_t *regs_out /* host [n][m] */);
/* device-resident form. plan = host-built launch plan (d2g_oph_plan_*); all other pointers device. */
typedef struct d2g_oph_plan d2g_oph_plan;
int  d2g_oph_plan_create(d2g_ctx *ctx, const uint64_t *run_start, const uint32_t *run_len, size_t nrun,
                         const uint64_t *genome_run_off, size_t n, int k, d2g_oph_plan **out);
void d2g_oph_plan_destroy(d2g_oph_plan *plan);
uint64_t d2g_oph_plan_nkmers(const d2g_oph_plan *plan);   /* total k-mers the plan covers: emissions (window positions under a window) */

/* ---- K1w: windowed minimizers, -w / --window-size -------------------------------
 * Replaces bns::Encoder<bns::score::Lex> over a Spacer(k, w) (reference d2.h:136, contain_main.cpp:34,185; the enumerator itself lives
 * in the absent bonsai and is restated from its published form: parity unpinned).  With w > k, q = w - k + 1: a run of valid bases
 * with k-mers x_0 .. x_{nk-1} has nk - q + 1 = len - w + 1 window positions (none when len < w); position i emits the ONE k-mer of
 * x_i .. x_{i+q-1} with the smallest score x ^ 0xe37e28c4271b5a2d (compared as uint64), once per position, duplicates included.
 * Nothing spans two runs.  The emitted k-mer stands for "a k-mer of the input" for everything downstream -- the filter test, the
 * OPH register, counts, the -m threshold, the exact counter, the distinct count, the screen's hit counters -- and every multiplicity
 * is a number of window positions.  w <= k (0 included) is no window: every k-mer, bit for bit as without one.
 * Cap: w - k <= 4095 (D2G_WINDOW_MAX_Q = 4096 k-mers per window); a wider window is D2G_ERR_UNSUPPORTED from the plan / the run.
 * A window is an attribute of a plan or a sketcher, like a filter: every d2g_*_dev call over a windowed plan and every
 * d2g_sketcher_run* (packed == NULL included), d2g_kmer_filter_create_dev and d2g_screen_add_dev / d2g_sketcher_run_screen honour it.
 * The one-shot host-pointer entry points (d2g_oph_sketch, ...) take none.  Runs are still cut at k: a run with k <= len < w is legal
 * and emits nothing.  A d2g_seqpack and the device parser know no window: their per-genome totals (d2g_seqpack_nkmers, genome_nkmers) stay
 * k-mer counts; d2g_oph_plan_nkmers and d2g_run_emissions give emissions.  A run longer than 2^30 bases is split by the packer into
 * pieces that overlap by k - 1 bases, so the windows across such a cut are not walked. */
#define D2G_WINDOW_MAX_Q 4096
/* host, no GPU: the k-mers a run of len valid bases emits under (k, w) -- the one count every layout and total follows from */
uint64_t d2g_run_emissions(uint64_t len, int k, int w);
/* d2g_oph_plan_create is the w = 0 form */
int  d2g_oph_plan_create_windowed(d2g_ctx *ctx, const uint64_t *run_start, const uint32_t *run_len, size_t nrun,
                                  const uint64_t *genome_run_off, size_t n, int k, int w, d2g_oph_plan **out);
uint64_t d2g_oph_plan_nbases(const d2g_oph_plan *plan);   /* total bases in the runs */

/* ---- K1a: amino-acid k-mers, --protein / --protein14 / --protein8 / --protein6 -------------------------------
 * Replaces bns::Encoder over a protein RollingHashingType (reference options.h:143-148,328-331; the encoder and the reduced
 * alphabets live in the absent bonsai and are restated as this library's own spec "D2G-AA": parity unpinned).  Ids and names are
 * those of the reference's python/parse.py:8-23.  A residue's code is the position of its group in the list:
 *   D2G_ALPHABET_PROTEIN20     A = 20   A C D E F G H I K L M N P Q R S T V W Y      k <= 14
 *   D2G_ALPHABET_PROTEIN_14    A = 14   A C D EQ FY G H IV KR LM N P ST W            k <= 16
 *   D2G_ALPHABET_PROTEIN_3BIT  A =  8   AST C DHN EKQR FWY G ILMV P                  k <= 21
 *   D2G_ALPHABET_PROTEIN_6     A =  6   AST CP DEHKNQR FWY G ILMV                    k <= 24
 * Letters of either case; any other byte (X B Z J U O * - included) and a record boundary end a run; runs shorter than k are
 * dropped.  The key of the k-mer with codes c_0 .. c_{k-1} is sum c_j A^(k-1-j) (first residue most significant), k at most the
 * largest with A^k <= 2^64; every key is below 2^63.  There is no canonical form: canon != 0 is D2G_ERR_INVALID.  The key then
 * takes the road of a DNA k-mer: Wang(x ^ xormask), OPH, counts, the filter table, the exact counter.
 * Stream layout: one byte per residue holding its code, runs back to back, >= 64 readable bytes behind the last residue, 4-byte
 * aligned; run_start / run_len count residues.
 * An alphabet is an attribute of a plan or a sketcher, like a window: every d2g_*_dev call over such a plan and every
 * d2g_sketcher_run* honour it; a k-mer filter records the alphabet it was built under and fits only calls under the same.  The
 * one-shot host-pointer entry points take none.  D2G_ERR_UNSUPPORTED: k > d2g_alphabet_max_k; a window w > k together with a
 * protein alphabet; d2g_sketcher_ingest_fasta (K0 parses DNA); d2g_sketcher_run_screen / d2g_screen_add_dev. */
#define D2G_ALPHABET_DNA 0
#define D2G_ALPHABET_PROTEIN20 2
#define D2G_ALPHABET_PROTEIN_3BIT 3
#define D2G_ALPHABET_PROTEIN_14 4
#define D2G_ALPHABET_PROTEIN_6 5
/* host, no GPU.  Symbols of the alphabet (4 for DNA; 0 for an unknown id), the largest k (32 for DNA; 0), the code of a byte or
 * -1, the reference's name ("DNA", "PROTEIN20", "PROTEIN_3BIT", "PROTEIN_14", "PROTEIN_6"; "" for an unknown id) */
int         d2g_alphabet_size(int alphabet);
int         d2g_alphabet_max_k(int alphabet);
int         d2g_alphabet_code(int alphabet, int byte);
const char *d2g_alphabet_name(int alphabet);
/* bits of the widest key of (k, alphabet): 2k for DNA, the bit length of A^k - 1 otherwise; 0 when k is outside [1, max k] */
int         d2g_key_bits(int k, int alphabet);
/* d2g_oph_plan_create is the alphabet-0 form; runs count residues */
int  d2g_oph_plan_create_alphabet(d2g_ctx *ctx, const uint64_t *run_start, const uint32_t *run_len, size_t nrun,
                                  const uint64_t *genome_run_off, size_t n, int k, int alphabet, d2g_oph_plan **out);
int  d2g_oph_sketch_dev(d2g_ctx *ctx, const d2g_oph_plan *plan, const uint8_t *packed_dev,
                        int canon, uint64_t xormask, size_t sketchsize,
                        uint64_t *regs_out_dev /* [n][m] */, void *stream);

/* K1b: how often the k-mer behind each register occurred -- LazyOnePermSetSketch's counts_ / idcounts() (reference
 * src/oph.h:207-209,272-277; call site src/fastxsketch.cpp:590-591,621-622).  counts_out[g][r] = number of k-mers of genome g whose
 * OPH id equals regs[g][r] and maps to register r; defined for ANY regs, not only K1's output (a value no k-mer has counts 0).
 * An empty register (~0) is compared like any other value: a k-mer whose id is 2^64-1 counts, as in the reference.
 * Writes every word of [n][m]; launched on `stream` (after the launch that produced regs), does not synchronise. */
int  d2g_oph_count_dev(d2g_ctx *ctx, const d2g_oph_plan *plan, const uint8_t *packed_dev,
                       int canon, uint64_t xormask, size_t sketchsize,
                       const uint64_t *regs_dev /* [n][m] */, uint32_t *counts_out_dev /* [n][m] */, void *stream);
/* K1, then the count pass over K1's registers: d2g_oph_sketch's inputs and registers, plus the counts.  A genome with 2^32
 * k-mers or more is D2G_ERR_UNSUPPORTED (the reference's uint32 copy of its counts wraps there; that is not reproduced). */
int d2g_oph_sketch_counts(d2g_ctx *ctx, const uint8_t *packed, size_t packed_bytes,
                          const uint64_t *run_start, const uint32_t *run_len, size_t nrun,
                          const uint64_t *genome_run_off, size_t n,
                          int k, int canon, uint64_t xormask, size_t sketchsize,
                          uint64_t *regs_out /* host [n][m] */, uint32_t *counts_out /* host [n][m] */);

/* persistent form for host ingest pipelines: grow-only device buffers, one pinned-arena upload of
 * the launch tables per call, own stream.  Same arguments and result as d2g_oph_sketch. */
typedef struct d2g_sketcher d2g_sketcher;
int  d2g_sketcher_create(d2g_ctx *ctx, d2g_sketcher **out);
void d2g_sketcher_destroy(d2g_sketcher *sk);
/* K1w (above): every later d2g_sketcher_run* of this sketcher walks the minimizers of windows of w bases when w > its k; 0, or any
 * w <= k, switches the window off.  A w beyond the cap is refused by the run (it is the run that knows k). */
int  d2g_sketcher_set_window(d2g_sketcher *sk, int w);
/* K1a (above): every later d2g_sketcher_run* of this sketcher reads its stream as one byte per residue of this alphabet;
 * D2G_ALPHABET_DNA switches back.  An unknown id is D2G_ERR_INVALID. */
int  d2g_sketcher_set_alphabet(d2g_sketcher *sk, int alphabet);
int  d2g_sketcher_run(d2g_sketcher *sk, const uint8_t *packed, size_t packed_bytes,
                      const uint64_t *run_start, const uint32_t *run_len, size_t nrun,
                      const uint64_t *genome_run_off, size_t n, int k, int canon, uint64_t xormask,
                      size_t sketchsize, uint64_t *regs_out /* host [n][m] */);

/* the same with the counts of d2g_oph_sketch_counts (packed == NULL after d2g_sketcher_ingest_fasta works as for d2g_sketcher_run) */
int  d2g_sketcher_run_counts(d2g_sketcher *sk, const uint8_t *packed, size_t packed_bytes,
                             const uint64_t *run_start, const uint32_t *run_len, size_t nrun,
                             const uint64_t *genome_run_off, size_t n, int k, int canon, uint64_t xormask,
                             size_t sketchsize, uint64_t *regs_out /* host [n][m] */, uint32_t *counts_out /* host [n][m] */);

/* ---- K3o: sketch -m c in set space: registers over the k-mers seen at least c times ----
 * LazyOnePermSetSketch under set_mincount(c) (reference src/oph.h:154-159,188-205; src/fastxsketch.cpp:192).  Its per-register map of
 * candidates ends, whatever the order of the k-mers, at: register r = the smallest OPH id among the DISTINCT k-mers that map to r and
 * occur >= c times (~0 if none); counts r = every occurrence of the k-mer whose id equals the final register -- what d2g_oph_count_dev
 * defines for any registers (so an empty register counts the occurrences of a k-mer whose id is 2^64-1, even fewer than c).
 * The input's k-mers are counted exactly by K3's bucketed LDS tables (a filter's k-mers do not count towards c), the selection is the
 * new kernel k3_ophmin_kernel, the counts are K1b over the new registers on the same stream.  Note the convention: this keeps
 * count >= c, --multiset's count_threshold keeps count > threshold (src/counter.h:124).
 * mincount < 2 is the plain sketch: what d2g_sketcher_run / _run_counts (d2g_oph_sketch_dev) return, bit for bit.
 * counts_out may be NULL (no count pass); with it, a genome of 2^32 k-mers or more is refused as by d2g_oph_sketch_counts.  Null
 * regs_out with n > 0 and a sketchsize out of range are D2G_ERR_INVALID before anything is written; n = 0 is D2G_OK.
 * The _dev form synchronises `stream` before it returns (the status word of the kernels is checked), like d2g_bmh_sketch_dev;
 * counts for it: d2g_oph_count_dev over regs_out_dev. */
int d2g_oph_sketch_mincount(d2g_ctx *ctx, const uint8_t *packed, size_t packed_bytes,
                            const uint64_t *run_start, const uint32_t *run_len, size_t nrun,
                            const uint64_t *genome_run_off, size_t n,
                            int k, int canon, uint64_t xormask, size_t sketchsize, uint32_t mincount,
                            uint64_t *regs_out /* host [n][m] */, uint32_t *counts_out /* host [n][m] or NULL */);
int d2g_oph_sketch_mincount_dev(d2g_ctx *ctx, const d2g_oph_plan *plan, const uint8_t *packed_dev,
                                int canon, uint64_t xormask, size_t sketchsize, uint32_t mincount,
                                uint64_t *regs_out_dev /* [n][m] */, void *stream);
/* persistent form (packed == NULL after d2g_sketcher_ingest_fasta works as for d2g_sketcher_run) */
int d2g_sketcher_run_mincount(d2g_sketcher *sk, const uint8_t *packed, size_t packed_bytes,
                              const uint64_t *run_start, const uint32_t *run_len, size_t nrun,
                              const uint64_t *genome_run_off, size_t n, int k, int canon, uint64_t xormask,
                              size_t sketchsize, uint32_t mincount,
                              uint64_t *regs_out /* host [n][m] */, uint32_t *counts_out /* host [n][m] or NULL */);

/* ---- K1f: --filterset, k-mers that every sketch skips ---------------------------
 * Replaces FilterSet in its sorted-hash-set form (reference src/filterset.h:35-222, built at src/d2.cpp:45-98) and its test
 * `if(!opts.fs_ || !opts.fs_->in_set(maskfn(x))) func(maskfn(x))` (src/fastxsketch.cpp:385-398, src/fastxsketchbyseq.cpp:327,370,383):
 * the k-mers of the filter input -- enumerated exactly as a sketch input's are, with the sketch's k and canonicalisation -- sit in an
 * open-addressing table in device memory, and the k-mer walker of K1, K1b and K3 hands on only the k-mers that are NOT in it.  A
 * filtered k-mer is invisible to everything downstream: OPH registers, their counts, the exact counter behind --multiset (registers,
 * total weight, the count threshold applied to what remains) and the distinct count; an input whose k-mers are all filtered behaves
 * like an input without k-mers.  The table holds RAW 2-bit k-mers (maskfn is a bijection), so it does not depend on the seed or
 * xormask of the sketch calls; it does depend on k and canon.  A filter without k-mers is legal and filters nothing. */
typedef struct d2g_kmer_filter d2g_kmer_filter;
/* device-resident: plan + packed stream of the filter input (all its "genomes" go into ONE set); enqueues on stream */
int  d2g_kmer_filter_create_dev(d2g_ctx *ctx, const d2g_oph_plan *plan, const uint8_t *packed_dev, int canon, void *stream,
                                d2g_kmer_filter **out);
/* host-pointer form: the packed-run-stream arguments of d2g_oph_sketch (so a d2g_seqpack feeds it); synchronises */
int  d2g_kmer_filter_create(d2g_ctx *ctx, const uint8_t *packed, size_t packed_bytes, const uint64_t *run_start, const uint32_t *run_len,
                            size_t nrun, int k, int canon, d2g_kmer_filter **out);
/* the same under a window (K1w): the filter input is enumerated with it, noccurrences counts its emissions; w <= k: no window */
int  d2g_kmer_filter_create_windowed(d2g_ctx *ctx, const uint8_t *packed, size_t packed_bytes, const uint64_t *run_start,
                                     const uint32_t *run_len, size_t nrun, int k, int canon, int w, d2g_kmer_filter **out);
/* the same under a protein alphabet (K1a): a byte-per-residue stream, no canonical form, no window.  A filter records its alphabet and
 * fits only plans and sketchers under the same one */
int  d2g_kmer_filter_create_alphabet(d2g_ctx *ctx, const uint8_t *packed, size_t packed_bytes, const uint64_t *run_start,
                                     const uint32_t *run_len, size_t nrun, int k, int alphabet, d2g_kmer_filter **out);
void d2g_kmer_filter_destroy(d2g_kmer_filter *filter);
/* k-mer occurrences put in (duplicates counted: the reference's data_.size()), distinct keys held, bytes of the device table;
 * synchronises the device */
int  d2g_kmer_filter_info(d2g_ctx *ctx, const d2g_kmer_filter *filter, uint64_t *noccurrences, uint64_t *ndistinct, size_t *table_bytes);
/* membership of n raw 2-bit k-mers (host arrays; canonical ones for a canon filter), through the SAME device probe the walker uses */
int  d2g_kmer_filter_contains(d2g_ctx *ctx, const d2g_kmer_filter *filter, const uint64_t *kmers, size_t n, uint8_t *out);
/* attach (NULL detaches).  The filter must outlive the plan / sketcher or be detached first.  A filter of another context, k,
 * canon or window (a filter remembers the window it was built under, 0 = none) makes the SKETCH call return D2G_ERR_INVALID, before it writes anything.  More than 2^31 k-mers: D2G_ERR_UNSUPPORTED at
 * creation; no memory for the table: D2G_ERR_NOMEM (never a smaller table).
 * A plan's filter is honoured by d2g_oph_sketch_dev, d2g_oph_count_dev, d2g_oph_sketch_mincount_dev, d2g_bmh_sketch_dev and d2g_kmer_sets_dev; a sketcher's by every
 * d2g_sketcher_run*, packed == NULL (K0-ingested) included.  --multiset calls with a filter walk the input once more, first, to count
 * the surviving k-mers per genome (their layout depends on it) and wait for that count.  The one-shot host-pointer entry points
 * (d2g_oph_sketch, d2g_bmh_sketch, d2g_kmer_count, ...) take no filter. */
int  d2g_oph_plan_set_filter(d2g_oph_plan *plan, const d2g_kmer_filter *filter);
int  d2g_sketcher_set_filter(d2g_sketcher *sk, const d2g_kmer_filter *filter);

/* ---- K1s: `dashing2 contain`, reads screened against a database of sampled k-mers ----
 * Replaces the reference's mash-screen loop (src/contain_main.cpp:34-59,188-244): kmer2ids.find(maskfn(kmer)) once per k-mer of
 * every query, then per (query, reference) the number of the reference's S sampled keys that occur in the query and how often.
 * A d2g_screen is resident on the device: the distinct keys of the database (keys[nrefs][S], MASKED: maskfn(kmer) =
 * d2g_wang_hash(kmer ^ xormask), the payload of the <out>.kmer64 that `sketch -s` writes) in K1f's table of raw k-mers, a dense id
 * per key, the id of every database position, and u32 counters cnt[nrows][ndistinct] -- one row per query the caller wants to keep
 * apart.  Counters are zero at creation and after d2g_screen_reset, and ADDITIVE over calls: a query may be fed in pieces.
 * Per (row q, reference r):  matches = #{ j : cnt[q][id(key[r][j])] > 0 },  matchsum = sum_j cnt[q][id(key[r][j])] mod 2^32
 * (a key that stands in two registers of r counts twice, as in the reference: in practice the key of an empty register).
 * The screen counts the k-mers fed to each row on the host; a call that would take a row to 2^32 k-mers or beyond returns
 * D2G_ERR_UNSUPPORTED before it enqueues anything -- below that no counter can wrap.
 * nrefs == 0 is legal.  Not enough device memory: D2G_ERR_NOMEM with the bytes needed and free in d2g_last_error, never a smaller
 * table.  More than D2G_SCREEN_MAX_KEYS = 2^30 database keys (nrefs x S): D2G_ERR_UNSUPPORTED before anything is ranked -- the table
 * would pass 2^31 slots, and the walker's probe names a slot in 32 bits with two values set aside (not found; the all-ones k-mer). */
#define D2G_SCREEN_MAX_KEYS (1ull << 30)
typedef struct d2g_screen d2g_screen;
/* host, no GPU: the slots of the table of a screen with `ndistinct` distinct keys (the power of two >= 2 ndistinct, >= 16, <= 2^31);
 * D2G_ERR_UNSUPPORTED and *slots = 0 beyond D2G_SCREEN_MAX_KEYS */
int  d2g_screen_table_slots(uint64_t ndistinct, uint64_t *slots);
int  d2g_screen_create(d2g_ctx *ctx, const uint64_t *keys /* host [nrefs][S] */, size_t nrefs, size_t sketchsize, int k, int canon,
                       uint64_t xormask, size_t nrows, d2g_screen **out);
void d2g_screen_destroy(d2g_screen *screen);
/* every counter back to zero, every row's k-mer tally too; synchronises the device */
int  d2g_screen_reset(d2g_ctx *ctx, d2g_screen *screen);
/* distinct keys held, bytes of the device table (keys + ids), bytes of the counters */
int  d2g_screen_info(d2g_ctx *ctx, const d2g_screen *screen, uint64_t *ndistinct, size_t *table_bytes, size_t *counter_bytes);
/* the k-mers fed to a row since the last reset: what the 2^32 guard reads.  d2g_screen_set_fed overwrites the tally (the counters
 * are not touched): a caller that restores a checkpoint, and the tests of the guard. */
int  d2g_screen_fed(d2g_ctx *ctx, const d2g_screen *screen, size_t row, uint64_t *nkmers);
int  d2g_screen_set_fed(d2g_ctx *ctx, d2g_screen *screen, size_t row, uint64_t nkmers);
/* device-resident form: the k-mers of genome g of the plan count towards row genome_row[g] (host array [n]; several genomes may
 * share a row, several rows a launch).  The k-mers are enumerated with the plan's k and the SCREEN's canonicalisation; a plan's
 * filter plays no part (one that does not fit the call is refused, as a sketcher's is).  Enqueues on `stream`, does not synchronise; calls on one screen go to one stream or are ordered by the
 * caller.  A screen of another context or k: D2G_ERR_INVALID before anything is written. */
int  d2g_screen_add_dev(d2g_ctx *ctx, d2g_screen *screen, const d2g_oph_plan *plan, const uint8_t *packed_dev,
                        const uint32_t *genome_row /* host [n] */, void *stream);
/* sketcher form: the packed-run arguments of d2g_sketcher_run (packed == NULL after d2g_sketcher_ingest_fasta works as there), so a
 * d2g_seqpack and the K0 device parser feed it; synchronises.  A screen of another context, k or canon: D2G_ERR_INVALID before
 * anything is written.  The sketcher's filter plays no part. */
int  d2g_sketcher_run_screen(d2g_sketcher *sk, const uint8_t *packed, size_t packed_bytes,
                             const uint64_t *run_start, const uint32_t *run_len, size_t nrun,
                             const uint64_t *genome_run_off, size_t n, int k, int canon,
                             d2g_screen *screen, const uint32_t *genome_row /* host [n] */);
/* matches and matchsums of rows [row0, row0 + nrows) against every reference; synchronises the device */
int  d2g_screen_result(d2g_ctx *ctx, const d2g_screen *screen, size_t row0, size_t nrows,
                       uint32_t *matches_out /* host [nrows][nrefs] */, uint32_t *matchsums_out /* host [nrows][nrefs] */);
/* the counters themselves: the distinct MASKED keys in ascending order and row `row`'s count of each (either may be NULL);
 * synchronises the device */
int  d2g_screen_key_counts(d2g_ctx *ctx, const d2g_screen *screen, size_t row, uint64_t *keys_out /* [ndistinct] */,
                           uint32_t *counts_out /* [ndistinct] */);
/* host, no GPU (reference src/contain_main.cpp:221,237-241): coverage = (float)((1.0 / S) * matches) -- the product in double --
 * and depth = (float)(matchsum / matches), the INTEGER quotient of the two uint32; both 0 where matches == 0 */
int  d2g_epilogue_contain(const uint32_t *matches, const uint32_t *matchsums, size_t n, size_t sketchsize,
                          float *coverage_out /* [n] */, float *depth_out /* [n] */);

/* ---- K0: FASTA bytes -> packed run stream on the GPU (host ingest pipelines) ------
 * Replaces, for plain FASTA inputs, the host parser + 2-bit packer (d2g_seqpack_*; reference call sites
 * src/fastxsketch.cpp:383-424, src/d2.h:273-305): the caller read()s the files into ONE host buffer (page-locked memory from
 * d2g_malloc_host makes the upload a single DMA), file f at raw + file_off[f] (16-byte aligned), file_len[f] bytes; genome g =
 * files [genome_file_off[g], genome_file_off[g+1]) (several files can feed one sketch, like a reference input line with
 * spaces).  The packed stream stays in the sketcher's device buffer; the run table comes back to the host.  Then
 * d2g_sketcher_run / d2g_sketcher_run_bmh / d2g_sketcher_run_distinct with packed == NULL and the table of
 * d2g_sketcher_ingested_runs sketch it: registers bit-identical to the host-parsed path.
 * Returns D2G_ERR_UNSUPPORTED for what only the host parser handles: inputs that do not begin with '>' (gzip members, FASTQ,
 * leading junk), lines that begin with '+' (FASTQ quality sections, found only after the device passes have run), files of 2 GiB
 * and more.  After ANY failed ingest the sketcher's device stream is INVALID -- whatever an earlier ingest left there has been
 * overwritten or discarded -- and d2g_sketcher_run* with packed == NULL fails until the next successful ingest: re-stage.
 * The pointers of d2g_sketcher_ingested_runs stay valid until the next ingest on this sketcher. */
int d2g_sketcher_ingest_fasta(d2g_sketcher *sk, const uint8_t *raw, size_t raw_bytes, const uint64_t *file_off,
                              const uint64_t *file_len, size_t nfiles, const uint64_t *genome_file_off /* [n+1] */, size_t n, int k);
int d2g_sketcher_ingested_runs(const d2g_sketcher *sk, const uint64_t **run_start, const uint32_t **run_len, size_t *nrun,
                               const uint64_t **genome_run_off /* [n+1] */, const uint64_t **genome_nkmers /* [n] */,
                               uint64_t *nbases /* bases in the stream */);

/* ---- K3: --multiset sketches: exact k-mer counts (R11) -> BagMinHash (R12) ------
 * Replaces, per input, the reference chain
 *   Counter::add(maskfn(kmer))          src/counter.h:68-77 ; src/fastxsketch.cpp:386,430
 *   Counter::finalize(bmh, threshold)   src/counter.h:118-138 (update(key, count) for count > threshold)
 *   BagMinHash2<double>::update/data/total_weight   (ABSENT dnbaker/sketch bmh.h; src/d2.h:247,
 *                                                    src/fastxsketch.cpp:443-445,477-487)
 * Inputs are the packed run stream of K1.  Outputs per genome: S doubles (the register minima)
 * and the total weight (= number of counted k-mers with count > threshold), which the reference
 * stores as the cardinality.  BagMinHash arithmetic follows the published algorithm under the
 * "BMH-D2G" spec in DESIGN.md: PARITY UNPINNED against a real dashing2 binary (its source is
 * absent), bit-exact against oracle/d2_bmh_oracle.c.  An input without k-mers yields +inf registers.
 */
int d2g_bmh_sketch(d2g_ctx *ctx, const uint8_t *packed, size_t packed_bytes,
                   const uint64_t *run_start, const uint32_t *run_len, size_t nrun,
                   const uint64_t *genome_run_off, size_t n,
                   int k, int canon, uint64_t xormask, size_t sketchsize, double count_threshold,
                   double *sig_out /* host [n][S] */, double *total_weight_out /* host [n] */);
/* device-resident form (plan and packed stream as for d2g_oph_sketch_dev); synchronises `stream`
 * before returning (the status word of the kernels is checked) */
int d2g_bmh_sketch_dev(d2g_ctx *ctx, const d2g_oph_plan *plan, const uint8_t *packed_dev,
                       int canon, uint64_t xormask, size_t sketchsize, double count_threshold,
                       double *sig_out_dev /* [n][S] */, double *total_weight_out_dev /* [n] */, void *stream);
/* persistent form (same buffers/stream as d2g_sketcher_run) */
int d2g_sketcher_run_bmh(d2g_sketcher *sk, const uint8_t *packed, size_t packed_bytes,
                         const uint64_t *run_start, const uint32_t *run_len, size_t nrun,
                         const uint64_t *genome_run_off, size_t n, int k, int canon, uint64_t xormask,
                         size_t sketchsize, double count_threshold,
                         double *sig_out /* host [n][S] */, double *total_weight_out /* host [n] */);
/* R11 alone (Counter::finalize(vector&, vector&, threshold), src/counter.h:78-117, minus the
 * sort): the distinct masked k-mers of genome g with count > threshold and their counts land in
 * keys_out/counts_out[genome_off_out[g] .. genome_off_out[g+1]) in unspecified order.
 * cap = capacity of the two output arrays (the total k-mer count always suffices). */
int d2g_kmer_count(d2g_ctx *ctx, const uint8_t *packed, size_t packed_bytes,
                   const uint64_t *run_start, const uint32_t *run_len, size_t nrun,
                   const uint64_t *genome_run_off, size_t n, int k, int canon, uint64_t xormask,
                   double count_threshold, uint64_t *keys_out, uint32_t *counts_out, size_t cap,
                   uint64_t *genome_off_out /* [n+1] */);
/* number of DISTINCT masked k-mers per genome (exact): the cardinality the reference substitutes for
 * small --parse-by-seq sketches (src/fastxsketchbyseq.cpp:415-430, `ids.size()`); same bucketed LDS
 * counting as d2g_kmer_count without materialising the keys on the host. */
int d2g_kmer_distinct(d2g_ctx *ctx, const uint8_t *packed, size_t packed_bytes,
                      const uint64_t *run_start, const uint32_t *run_len, size_t nrun,
                      const uint64_t *genome_run_off, size_t n, int k, int canon, uint64_t xormask,
                      uint64_t *ndistinct_out /* host [n] */);
int d2g_sketcher_run_distinct(d2g_sketcher *sk, const uint8_t *packed, size_t packed_bytes,
                              const uint64_t *run_start, const uint32_t *run_len, size_t nrun,
                              const uint64_t *genome_run_off, size_t n, int k, int canon, uint64_t xormask,
                              uint64_t *ndistinct_out /* host [n] */);
/* BagMinHash of explicit weighted sets (reference src/wsketch.cpp:54-73 minwise_det and 17-51
 * minhash_rowwise_csr: h.update(id, weight) per element): set i = elements
 * [set_off[i], set_off[i+1]); weights == NULL means 1.0; weights <= 0 are ignored (as
 * BagMinHash2::update does), weights above 2^53 or NaN are rejected, and so is a set whose total weight
 * is too small for the sketch size (d2g_bmh_check_weights). */
/* the host-side checks of d2g_bmh_from_weighted / _ids on their own (no context, no device): D2G_ERR_INVALID with a message
 * in err (may be NULL) for a NaN weight, a weight above 2^53, a set_off that is not monotone, a sketchsize outside
 * [1, 2^24), and for a non-empty set whose TOTAL weight W is too small for the sketch size: the first guess of its pruning
 * bound, scale * 1.25 (S / W) (ln S + 8.58), must be below 2^864 -- the walk raises a failed guess 16-fold at most 40 times
 * (16^40 = 2^160), and a bound that reached +inf would prune nothing and never end.  At scale 1 (the library's, unless
 * D2G_K3_GUESS_SCALE says otherwise) that refuses totals below about 1e-252 at S = 2^24 - 1 and about 1e-259 at S = 1;
 * single tiny weights inside a set of ordinary total are fine.  d2g_bmh_from_weighted / _ids run it first. */
int d2g_bmh_check_weights(const double *weights /* NULL = all 1.0 */, const uint64_t *set_off /* [nsets+1] */, size_t nsets,
                          size_t sketchsize, double scale, char *err, size_t errcap);
int d2g_bmh_from_weighted(d2g_ctx *ctx, const uint64_t *ids, const double *weights,
                          const uint64_t *set_off /* [nsets+1] */, size_t nsets, size_t sketchsize,
                          double *sig_out /* host [nsets][S] */, double *total_weight_out /* host [nsets] */);
/* the same + BagMinHash2::ids() (reference src/wsketch.cpp:36-37,66-67): owner_out[i][r] = position, within
 * set i, of the element whose point register r holds (the smaller position on an exact tie); ~0 for a
 * register no element reached (empty set).  owner_out may be NULL. */
int d2g_bmh_from_weighted_ids(d2g_ctx *ctx, const uint64_t *ids, const double *weights,
                              const uint64_t *set_off /* [nsets+1] */, size_t nsets, size_t sketchsize,
                              double *sig_out /* host [nsets][S] */, double *total_weight_out /* host [nsets] */,
                              uint64_t *owner_out /* host [nsets][S] or NULL */);

/* ---- K3k: --multiset -c/--countsketch-size/--countmin-size <cells>: approximate counts in a single-row count-sketch (R20) ----
 * Replaces, per input, Counter(cssize)::add(maskfn(kmer)) and ::finalize(bmh, threshold) (src/counter.h:16-19,68-77,131-137):
 *   hv = Wang(maskfn(x)) for every k-mer x the walker emits; table[hv % cells] += (hv >> 63) ? +1 : -1;
 *   then every cell i with |table[i]| >= threshold (>=, where the exact mode keeps count > threshold) and > 0 is the element
 *   (id = i, weight = |table[i]|) of BagMinHash (BMH-D2G, as d2g_bmh_from_weighted), total weight = the sum of those weights.
 * The cells are int32 on the device and hold the exact sums; the reference's float cells stop counting at 2^24.
 * Device memory: 4 * cells bytes per input whatever its length (K3 keeps 16 bytes per k-mer).  A batch whose tables do not fit a
 * sixth of the free device memory -- or D2G_CS_TABLE_BYTES, a debugging switch -- goes in groups of inputs; the output is the same.
 * Refused with D2G_ERR_INVALID before anything is staged or launched: cells outside [1, 2^31], an input of 2^31 k-mers or more;
 * with D2G_ERR_NOMEM before anything is launched: one table larger than the free device memory (the message has both figures).
 * The three forms of every K3 job; a sketcher's / plan's filter, window and alphabet are honoured as by d2g_sketcher_run_bmh /
 * d2g_bmh_sketch_dev.  An input without k-mers, or with every cell below the threshold: +inf registers, total weight 0. */
int d2g_bmh_sketch_cs(d2g_ctx *ctx, const uint8_t *packed, size_t packed_bytes,
                      const uint64_t *run_start, const uint32_t *run_len, size_t nrun,
                      const uint64_t *genome_run_off, size_t n,
                      int k, int canon, uint64_t xormask, size_t sketchsize, uint64_t cells, double count_threshold,
                      double *sig_out /* host [n][S] */, double *total_weight_out /* host [n] */);
/* synchronises `stream` before returning, like d2g_bmh_sketch_dev (and once per group and BagMinHash pass in between) */
int d2g_bmh_sketch_cs_dev(d2g_ctx *ctx, const d2g_oph_plan *plan, const uint8_t *packed_dev,
                          int canon, uint64_t xormask, size_t sketchsize, uint64_t cells, double count_threshold,
                          double *sig_out_dev /* [n][S] */, double *total_weight_out_dev /* [n] */, void *stream);
int d2g_sketcher_run_bmh_cs(d2g_sketcher *sk, const uint8_t *packed, size_t packed_bytes,
                            const uint64_t *run_start, const uint32_t *run_len, size_t nrun,
                            const uint64_t *genome_run_off, size_t n, int k, int canon, uint64_t xormask,
                            size_t sketchsize, uint64_t cells, double count_threshold,
                            double *sig_out /* host [n][S] */, double *total_weight_out /* host [n] */);
/* the first two stages on their own (tests, integrators).  The signed tables, dense: at most 2^28 cells in all */
int d2g_countsketch_table(d2g_ctx *ctx, const uint8_t *packed, size_t packed_bytes,
                          const uint64_t *run_start, const uint32_t *run_len, size_t nrun,
                          const uint64_t *genome_run_off, size_t n, int k, int canon, uint64_t xormask,
                          uint64_t cells, int32_t *table_out /* host [n][cells] */);
/* ... and the compacted lists, any table size: input g's kept cells, ascending, in ids_out / w_out[set_off_out[g] .. set_off_out[g+1]);
 * total_out[g] = the sum of its weights.  cap = capacity of the two arrays (min(cells, k-mers) per input always suffices) */
int d2g_countsketch_cells(d2g_ctx *ctx, const uint8_t *packed, size_t packed_bytes,
                          const uint64_t *run_start, const uint32_t *run_len, size_t nrun,
                          const uint64_t *genome_run_off, size_t n, int k, int canon, uint64_t xormask,
                          uint64_t cells, double count_threshold, uint64_t *ids_out, double *w_out, size_t cap,
                          uint64_t *set_off_out /* [n+1] */, uint64_t *total_out /* [n] */);
/* L: tables of up to this many cells are accumulated in LDS per workgroup and flushed; larger ones take every add in global memory */
int d2g_countsketch_lds_cells(void);
/* since the context was made: the largest table allocated (bytes), the groups and the batches of all count-sketch calls */
int d2g_countsketch_stats(d2g_ctx *ctx, uint64_t *table_bytes, uint64_t *groups, uint64_t *batches);

/* ---- K1i: interval sets (BED), sketch / cmp --bed (R21) -------------------------
 * Replaces bed2sketch (reference src/bedsketch.cpp:36-56): every position i of every line `chrom <TAB> start <TAB> stop`, start <= i <
 * stop, is the element chrhash ^ i, chrhash = XXH3_64bits(chrom without a leading [cC]hr).
 *   set space       OPSetSketch::update(chrhash ^ i): id = Wang((chrhash ^ i) ^ d2g_oph_xor_const()) -- ONE Wang hash, no maskfn, no seed --
 *                   reg[id mod m] = min(.., id) with K1's index rule; finalised by d2g_oph_finalize like any K1 registers
 *   --multiset      Counter::add(chrhash ^ i, inc), inc = 1 or 1 / (stop - start) (--normalize-intervals); the weight of a position is
 *                   the sum, in line order, of the inc of every line that covers it; every (id, weight) goes to BagMinHash (BMH-D2G over
 *                   the unhashed ids, as d2g_bmh_from_weighted).  Weights are summed per (chrhash, position): two chromosomes whose
 *                   hashes alias under ^ i stay two elements here (they merge in the reference's map).
 * Host half (no context): */
#define D2G_XXH3_MAX_LEN 240
/* XXH3_64bits (seed 0, default secret) of len <= D2G_XXH3_MAX_LEN bytes, restated from the published specification; a longer input
 * is not hashed: the result is 0 and callers check the length first (d2g_bed_parse refuses such a chromosome name) */
uint64_t d2g_xxh3_64(const void *data, size_t len);
/* The data lines of a BED buffer, in order: empty lines and lines that begin with '#' are skipped; the chromosome is what stands before
 * the first tab, less a leading chr / Chr when trim_chr; start and stop are two strtoul(p, &p, 10) calls on the rest of the line (a
 * missing field reads 0, "+5" is 5, a trailing CR is ignored).  At most `cap` lines are written to chrhash / start / stop (NULL with
 * cap 0: count only); *nlines is the number found (never more than the buffer's line feeds + 1).  D2G_ERR_INVALID with the text in err
 * (may be NULL): "Malformed line: <line>" for a line without a tab (the reference's words), a gzip magic at the buffer's start, a
 * chromosome name longer than D2G_XXH3_MAX_LEN bytes. */
int d2g_bed_parse(const char *buf, size_t len, int trim_chr, uint64_t *chrhash, uint64_t *start, uint64_t *stop, size_t cap,
                  size_t *nlines, char *err, size_t errcap);
/* Device half.  A plan over n files: file f owns lines [file_off[f], file_off[f+1]) of the three tables (host arrays, copied).  A lane
 * owns a chunk of at most 64 consecutive positions of ONE line, a workgroup chunks of ONE file; lines with start >= stop own nothing.
 * D2G_ERR_INVALID with nothing allocated: null tables, file_off not monotone or file_off[n] != nint;
 * D2G_ERR_UNSUPPORTED: a file with more than D2G_INTERVAL_MAX_POSITIONS positions (the message has the figure), 2^31 workgroups. */
#define D2G_INTERVAL_MAX_POSITIONS (1ull << 44)
typedef struct d2g_interval_plan d2g_interval_plan;
int  d2g_interval_plan_create(d2g_ctx *ctx, const uint64_t *chrhash, const uint64_t *start, const uint64_t *stop, size_t nint,
                              const uint64_t *file_off /* [n+1] */, size_t n, d2g_interval_plan **out);
void d2g_interval_plan_destroy(d2g_interval_plan *plan);
uint64_t d2g_interval_plan_npositions(const d2g_interval_plan *plan);   /* positions of all lines, overlaps counted */
/* K1i: registers [n][m], m = d2g_oph_m(sketchsize), pre-set to ~0 by the call; a file without positions keeps ~0.  The host form
 * synchronises; the _dev form enqueues on `stream` and returns (like d2g_oph_sketch_dev).  A plan of another context, a null output
 * (n > 0) or a sketchsize out of range: D2G_ERR_INVALID before anything is written. */
int  d2g_interval_oph_sketch(d2g_ctx *ctx, const d2g_interval_plan *plan, size_t sketchsize, uint64_t *regs_out /* host [n][m] */);
int  d2g_interval_oph_sketch_dev(d2g_ctx *ctx, const d2g_interval_plan *plan, size_t sketchsize, uint64_t *regs_out_dev /* [n][m] */,
                                 void *stream);
/* --multiset: a host sweep per file gives the maximal runs (chrhash, lo, hi, weight) -- chromosome hashes ascending, positions
 * ascending, the weight summed over the covering lines in line order; k1i_expand_kernel writes them out as (id, weight) lists on the
 * device (16 bytes per covered position), BagMinHash runs over the lists where they lie.  total_weight_out[f] = the sum, in run order,
 * of weight * positions.  Files go to the device in groups that fit a third of the free memory; one file that does not fit is
 * D2G_ERR_NOMEM with the bytes needed and the bytes free.  normalize != 0: inc = 1.0 / (double)(stop - start).  Synchronises. */
int  d2g_interval_bmh_sketch(d2g_ctx *ctx, const d2g_interval_plan *plan, int normalize, size_t sketchsize,
                             double *sig_out /* host [n][S] */, double *total_weight_out /* host [n] */);
/* the runs of the sweep on their own (host, no device work; tests): runs of file f in [run_off_out[f], run_off_out[f+1]); cap = capacity
 * of the four arrays; *nruns = the runs found (nothing beyond cap is written) */
int  d2g_interval_runs(const d2g_interval_plan *plan, int normalize, uint64_t *hash_out, uint64_t *lo_out, uint64_t *hi_out,
                       double *w_out, size_t cap, uint64_t *run_off_out /* [n+1] */, size_t *nruns);

/* ---- K2: dense all-pairs comparison -------------------------------------------
 * Replaces HOT LOOP B: emit_rectangular's row loops calling compare()
 * (reference src/emitrect.cpp:211-323 ; src/cmp_core.cpp:349-361,458-517).
 * sig_bits = the N x S signature matrix as raw 64-bit patterns (the doubles of
 * SketchingResult::signatures_, or u64 k-mer ids), row-major.  Equality of the bit
 * patterns == equality of the doubles (all signatures are >= +0.0 and never NaN).
 *
 * "ut" = condensed upper triangle in the reference's order (0,1),(0,2)...(0,N-1),(1,2)...
 * restricted to rows [r0, r1): out has sum_{r=r0}^{r1-1} (N-r-1) entries.
 */
size_t d2g_ut_count(size_t N, size_t r0, size_t r1);
/* prepared operand for repeated / sharded comparisons (device resident) */
typedef struct d2g_cmp_set d2g_cmp_set;
int  d2g_cmp_set_create_dev(d2g_ctx *ctx, const uint64_t *sig_bits_dev, size_t N, size_t sketchsize,
                            int algo, void *stream, d2g_cmp_set **out);
int  d2g_cmp_set_create(d2g_ctx *ctx, const uint64_t *sig_bits_host, size_t N, size_t sketchsize,
                        int algo, d2g_cmp_set **out);
/* re-load an existing set with a new N x S matrix of the same shape, reusing every device
 * buffer (no allocation; the whole prepare chain is enqueued on `stream`.  The FIRST prepare of a BITSLICE set of 8192 sketches or more -- and the
 * first after d2g_cmp_set_forget -- waits a few tens of microseconds for two small kernels that look at the matrix: INTEGRATION.md section 2) */
int  d2g_cmp_set_update_dev(d2g_ctx *ctx, d2g_cmp_set *set, const uint64_t *sig_bits_dev, void *stream);
/* The `_dev` prepare chain is asynchronous and cannot report a data-dependent failure when it is
 * enqueued.  The one such failure: a register column that puts more distinct values into one hash
 * partition of the bit-sliced prepare than its LDS table holds (N > 21 845 and an adversarial or
 * extremely skewed column; impossible for hashed registers).  d2g_cmp_set_status synchronises `stream`
 * and returns D2G_ERR_INTERNAL in that case (results computed from the set are then invalid; re-create
 * it with D2G_CMP_DIRECT).  The host-pointer entry points (d2g_cmp_set_create, d2g_cmp_eqcount_ut,
 * d2g_cmp_dist_ut) check it themselves and fall back to the direct algorithm under D2G_CMP_AUTO. */
int  d2g_cmp_set_status(d2g_ctx *ctx, const d2g_cmp_set *set, void *stream);
/* bit-sliced sets: max over register columns of (#values occurring >= 2 times) + 1 (values that
 * occur once are coded 0 in the row operand and all-ones in the column operand), the largest id-plane
 * count of any 32-register group and the mean over groups (each group only walks its own planes).
 * Synchronises `stream` and returns d2g_cmp_set_status's error, if any; all 0 for a DIRECT set. */
int  d2g_cmp_set_planes(d2g_ctx *ctx, const d2g_cmp_set *set, void *stream, unsigned *max_distinct, int *nbits,
                        float *mean_nbits);
/* width of the words a bit-sliced set keeps its per-column ids in between the kernels of its prepare: 16 for a set of N <= 21 845 sketches (the
 * rank kernel is single-partition: an id is 0, the unique flag 0x8000 or a rank 1 .. N / 2), 32 for larger sets, for sets whose ids are re-derived from
 * exchanged planes and everywhere under D2G_BS_ID16=0 (A/B measurements, tests); 0 for a set that keeps no ids (DIRECT sets, sets of truncated codes,
 * gathered operands without a sparse path).  Results do not depend on it. */
int  d2g_cmp_set_id_bits(const d2g_cmp_set *set);
/* Sparse tiles + pair list (bit-sliced sets of N >= 8192 sketches, owning sets and the multi-GPU engine's gathered operand;
 * D2G_BS_SPARSE=0 switches it off, D2G_BS_SPARSE_MIN_N moves the threshold): an equality count is 0 unless the two sketches share a
 * value in some register column.  The prepare finds the families (sketches that agree in MANY registers; a single chance collision
 * does not weld two families together), puts every family on adjacent positions and lists every pair of DIFFERENT families that
 * shares a value; an upper-triangle launch pre-fills the output with the value of "0 equal", walks only the 32 x 256 tiles a family's
 * rows and columns meet in and adds the listed pairs -- or, when that would not pay (one family holds most sketches, the families'
 * tiles are more than a third of all tiles, the list outgrows pairs / 4 entries), the plain kernel over every tile; decided on the
 * device, no host round trip.  Results are identical either way.
 * A sparse launch uses scratch of the set (work list, launch rows, control words): upper-triangle launches on ONE set must be issued
 * one after the other on ONE stream (rectangular launches and launches on different sets are independent).
 * info4 of the LAST upper-triangle launch on the set (synchronises `stream`): [0] 1 = the set has a sorted operand, [1] tiles
 * listed, [2] flags (bit 0: the prepare decided for the dense walk, bit 1: the dense kernel ran, bit 2: tiles + pair list were used,
 * bit 3: the caller's order was kept, bit 4: the prepare skipped the ordering because the previous prepare of this set had given up --
 * remembered per set, retried every 16th prepare, D2G_SP_REMEMBER=0 switches it off), [3] entries of the pair list (one per pair of
 * different families and shared value). */
int  d2g_cmp_set_sparse_info(d2g_ctx *ctx, const d2g_cmp_set *set, void *stream, uint32_t *info4);
/* diagnostics of the last prepare (synchronises `stream`): up to `cap` entries of the pair list (i | j << 32, i < j) and, if root_out is not null, the family
 * root of every sketch (sketches with equal roots sit in one segment).  Nothing in the product reads these back; tools/plist_stats.py does. */
int  d2g_cmp_set_debug_pairs(d2g_ctx *ctx, const d2g_cmp_set *set, void *stream, uint64_t *pairs_out, size_t cap, size_t *npairs, uint32_t *root_out);
/* diagnostics of the last prepare's sparse path (synchronises `stream`; all 0 for a set without one): [0] 1 = the prepare took the first look at its
 * matrix (sixteen sampled sketches against all), [1] 1 = the first look decided for the dense walk, [2..5] that look's raw sums (0 without one): register
 * counts below 4 (E), pairs at 4 or more (F), shared values over all columns, id planes over all columns; [6] 1 = the pair list went through
 * the binned + composed form, [7] the set's bin width (log2 of the columns of a chunk), [8] the schedule of the last prepare: 1 = merged (column plan and
 * planes inside launches of the ordering: the planes beside flatten), 2 = merged with the planes behind the pair-list kernel's workgroups (the default,
 * D2G_K2_MERGE=2), 0 = classic (kernel by kernel: D2G_K2_MERGE=0, a first look, a remembered give-up, the table form of the link
 * passes, split rank passes), [9] the kernels that prepare enqueued, the transpose included.  out10: TEN words.  Nothing in the product reads these back. */
int  d2g_cmp_set_sparse_detail(d2g_ctx *ctx, const d2g_cmp_set *set, void *stream, uint64_t *out10);
/* what became of the output announced to the set's last prepare (d2g_cmp_ut_announce_dev), in pieces of 32 KB: [0] the pieces announced (0: nothing was
 * announced, or it was cancelled), [1] those the rank kernel's own threads wrote (bit 64 of D2G_SP_RIDE; the single-partition register kernel, N <= 12 288,
 * on a prepare whose path is known when it is enqueued), [2] those the prepare's other kernels carried (rider workgroups; the side stream of an output of
 * 1 GB and more), [3] those left to the launch.  [1] + [2] + [3] = [0].  Host bookkeeping only: nothing is synchronised, no stream is touched; all 0 for a
 * set without a sparse path.  out4: FOUR words.  Nothing in the product reads these back. */
int  d2g_cmp_set_fill_detail(d2g_ctx *ctx, const d2g_cmp_set *set, uint64_t *out4);
/* the output bins of the pair list of a set of N sketches (bands of 32 rows x chunks of 2^cshift columns): what a set's allocation computes.
 * binned_ok = 0: more bands than bins fit, the list is applied entry by entry (nbins = 0).  Host arithmetic, no context. */
int  d2g_sparse_bin_geometry(size_t N, uint32_t *cshift, uint32_t *nch, uint32_t *nbins, int *binned_ok);
/* ---- sharded prepare (multi-GPU).  The bit-sliced operand is an array of independent
 * 32-register groups of `group_words` u32 each (+ one u32 of meta per group) whose geometry depends
 * on N only, so ranks can each build the groups of their own column slice and all-gather them:
 *   rows held by rank r --d2g_pack_column_slices_dev--> all-to-all --> column slice [N][S/W]
 *   --d2g_cmp_set_create_dev(N, S/W, BITSLICE)--> d2g_cmp_set_export_operand_dev --> all-gather
 *   --d2g_cmp_set_from_planes_dev(N, S, gathered)--> d2g_cmp_*_ut_dev on this rank's row range. */
int  d2g_operand_layout(size_t N, size_t sketchsize, size_t *group_words, size_t *ngroups);
int  d2g_cmp_set_export_operand_dev(d2g_ctx *ctx, const d2g_cmp_set *set, uint32_t *planes_out_dev,
                                    uint32_t *meta_out_dev, void *stream);
/* wraps a caller-owned (gathered) operand; only equality-count entry points work on it.  The operand may be
 * re-gathered into the same buffers between launches (its column coding is re-derived before every launch). */
int  d2g_cmp_set_from_planes_dev(d2g_ctx *ctx, size_t N, size_t sketchsize, const uint32_t *planes_dev,
                                 const uint32_t *meta_dev, d2g_cmp_set **out);
int  d2g_pack_column_slices_dev(d2g_ctx *ctx, const uint64_t *rows_dev, size_t n, size_t sketchsize, int nslices,
                                uint64_t *out_dev, void *stream);
void d2g_cmp_set_destroy(d2g_cmp_set *set);
int  d2g_cmp_set_algo(const d2g_cmp_set *set);      /* the algorithm actually selected */
/* equality counts (u32) for rows [r0,r1) of the upper triangle */
int  d2g_cmp_eqcount_ut_dev(d2g_ctx *ctx, const d2g_cmp_set *set, size_t r0, size_t r1,
                            uint32_t *neq_out_dev, void *stream);
/* fused table epilogue: out = lut[neq] (lut_dev: S+1 floats, see d2g_epilogue_lut) */
int  d2g_cmp_lut_ut_dev(d2g_ctx *ctx, const d2g_cmp_set *set, size_t r0, size_t r1,
                        const float *lut_dev, float *out_dev, void *stream);
/* The FILL of an upper-triangle launch, ahead of the launch.  From 8192 sketches on, a bit-sliced set's launch first fills its output
 * with the value of "no register equal" (200 MB at 10 000 sketches: 30 us at the HBM rate) and then writes the pairs that share
 * something.  The fill depends on nothing: a caller that knows the output before the operand is ready --
 * d2g_cmp_set_update_dev still to come, an exchange in flight -- enqueues it here, on ANY stream, and the NEXT upper-triangle launch
 * on the set into the same output and rows skips its own.  The caller orders the two: the same stream, or an event the launch's stream
 * waits for.  Exactly one of neq_out_dev / (lut_dev, out_dev) is given, as in the launch that follows.  A no-op for sets that would not
 * fill (small sets, the direct kernel); harmless when the launch decides for the dense walk (every output is written again). */
int  d2g_cmp_ut_prefill_dev(d2g_ctx *ctx, d2g_cmp_set *set, size_t r0, size_t r1, uint32_t *neq_out_dev,
                            const float *lut_dev, float *out_dev, void *stream);
/* The same fill with NO launch and NO stream of its own: the caller ANNOUNCES the output of the next upper-triangle launch before the
 * d2g_cmp_set_update_dev that precedes it, and that prepare's latency-bound kernels (one to forty workgroups each on an idle chip: column
 * plan, the counting sort of the families) carry the fill as extra workgroups behind their own.  Sequence per step:
 *     d2g_cmp_ut_announce_dev(ctx, set, r0, r1, ...);  d2g_cmp_set_update_dev(ctx, set, sigs, stream);  d2g_cmp_lut_ut_dev(..., stream);
 * The announcement serves exactly one prepare; the launch must follow on the prepare's stream with the same rows and output (any other
 * launch simply fills for itself).  lut_dev must hold the table by the time the prepare runs on its stream.  Nothing is enqueued here.
 * A no-op for sets that would not fill; D2G_SP_RIDE=0 turns the riding off (the launch fills as before); d2g_cmp_set_fill_detail says which
 * kernels of the prepare wrote how much of it.
 * The set keeps the announced pointer until its next prepare: a caller that frees the output before that prepare CANCELS the announcement
 * with neq_out_dev = out_dev = NULL.  A launch skips its own fill only where the announced (or pre-filled) output, rows AND fill value --
 * the count 0, or the table pointer -- are its own; a table whose first entry changes between the prepare and the launch is the caller's
 * business, as is a buffer written between the two. */
int  d2g_cmp_ut_announce_dev(d2g_ctx *ctx, d2g_cmp_set *set, size_t r0, size_t r1, uint32_t *neq_out_dev,
                             const float *lut_dev, float *out_dev);
/* measurements: the set forgets what its earlier prepares learnt about its matrix (which path pays); its next prepare decides as the first
 * prepare of a new set does */
int  d2g_cmp_set_forget(d2g_ctx *ctx, d2g_cmp_set *set);
/* (#a>b, #a<b) counts per pair: needs a set created with D2G_CMP_DIRECT (the raw patterns);
 * required when S is not a power of two in set space.  The order is that of the 64-bit patterns as
 * unsigned integers, which is the order of the doubles for non-negative, non-NaN registers (every
 * register the product writes) */
int  d2g_cmp_gtlt_ut_dev(d2g_ctx *ctx, const d2g_cmp_set *set, size_t r0, size_t r1,
                         uint32_t *gt_out_dev, uint32_t *lt_out_dev, void *stream);
/* rectangular block: rows [a0,a1) x cols [b0,b1) of the full N x N equality-count matrix,
 * row-major (asymmetric all-pairs = [0,N)x[0,N); panel = refs x queries). emitrect.cpp:211-268 */
int  d2g_cmp_eqcount_rect_dev(d2g_ctx *ctx, const d2g_cmp_set *set, size_t a0, size_t a1,
                              size_t b0, size_t b1, uint32_t *neq_out_dev, void *stream);

/* (#a>b, #a<b) for a rectangular block, a = row sketch, b = column sketch (compare(i,j) order);
 * the same unsigned 64-bit pattern order as d2g_cmp_gtlt_ut_dev */
int  d2g_cmp_gtlt_rect_dev(d2g_ctx *ctx, const d2g_cmp_set *set, size_t a0, size_t a1, size_t b0, size_t b1,
                           uint32_t *gt_out_dev, uint32_t *lt_out_dev, void *stream);

/* host-pointer conveniences (H2D, run, D2H, sync) */
int  d2g_cmp_eqcount_ut(d2g_ctx *ctx, const uint64_t *sig_bits, size_t N, size_t sketchsize,
                        size_t r0, size_t r1, int algo, uint32_t *neq_out);
/* full compare(): float distances for rows [r0,r1) with the reference's epilogue arithmetic.
 * cards = SketchingResult::cardinalities_; multiset_space selects cmp_core.cpp:495-517. */
int  d2g_cmp_dist_ut(d2g_ctx *ctx, const uint64_t *sig_bits, const double *cards, size_t N,
                     size_t sketchsize, size_t r0, size_t r1, int measure, int k, int multiset_space,
                     int algo, int nthreads, float *out);

/* ---- sets of truncated codes (d2g_regs_truncate) ----------------------------------------------------------------
 * codes = [N][S] unsigned integers of regbytes in {1, 2, 4}.  The device keeps them as 8 * regbytes bit planes (about
 * N * S * regbytes bytes, not N * S * 8); d2g_cmp_set_algo reports D2G_CMP_PLANES.  d2g_cmp_gtlt_ut_dev, d2g_cmp_gtlt_rect_dev,
 * d2g_cmp_eqcount_ut_dev and d2g_cmp_eqcount_rect_dev work on such a set (order = the codes as unsigned integers, eq = S - gt - lt);
 * d2g_cmp_lut_ut_dev, d2g_cmp_ut_prefill_dev, d2g_cmp_ut_announce_dev, d2g_cmp_set_export_operand_dev, d2g_cmp_set_update_dev and the
 * sparse diagnostics (d2g_cmp_set_sparse_info, _sparse_detail, _debug_pairs) return D2G_ERR_INVALID for it and write nothing. */
int  d2g_cmp_set_create_codes_dev(d2g_ctx *ctx, const void *codes_dev, size_t N, size_t sketchsize, int regbytes, void *stream,
                                  d2g_cmp_set **out);
int  d2g_cmp_set_create_codes(d2g_ctx *ctx, const void *codes_host, size_t N, size_t sketchsize, int regbytes, d2g_cmp_set **out);
/* bytes of device memory the set's operand occupies (any kind of set) */
size_t d2g_cmp_set_operand_bytes(const d2g_cmp_set *set);
/* host-pointer convenience: truncate (d2g_regs_truncate), upload, count, epilogue (d2g_epilogue_trunc_ut) for rows [r0,r1) of the
 * upper triangle.  sigs = densified double signatures [N][S]. */
int  d2g_cmp_dist_trunc_ut(d2g_ctx *ctx, const double *sigs, const double *cards, size_t N, size_t sketchsize, size_t r0, size_t r1,
                           int measure, int k, int regbytes, int bbit, int nthreads, float *out);

/* ---- K2e: nearest neighbours -- per-row selection on the device (cmp --topk / --similarity-threshold) ----------------
 * Replaces build_exact_graph (reference src/index_build.cpp:166-228) + the sign flip of src/cmp_core.cpp:787-793, for values that are
 * a MONOTONE function of the equality count (where d2g_epilogue_lut succeeds): both modes are then "list every j != i with
 * neq(i, j) >= t_i".  Only the listed neighbours leave the device, never the N x N matrix.  Always exhaustive (the reference's
 * EXACT_KNN=1 route), and ALL ties with the K-th best value are kept (the reference's stated intent, which its heap loop does
 * not reach: SURVEY F12).
 *
 * d2g_cmp_knn_dev, rows [r0, r1) of any kind of set: the counts of a band of `band_rows` rows x all N columns go into scratch of
 * the context (d2g_cmp_eqcount_rect_dev), then one workgroup per row selects.
 *   K == 0: threshold mode, t_i = min_count for every row (min_count = S + 1: nobody passes).
 *   K >= 1: top-K mode.  Only counts >= min_count are eligible (1 where a value of 0 is never a neighbour, 0 for distances);
 *           t_i = the K-th largest eligible count of row i, or min_count when the row has fewer than K eligible columns.
 *           cls_dev (may be NULL) = S + 1 words, cls[e] = the smallest count whose VALUE equals that of e: t_i is lowered to
 *           cls[t_i], so that a tie class of the K-th best value that spans several counts is kept whole.
 * The self pair is excluded by INDEX (duplicates list each other).  Row i - r0 owns slots [(i - r0) cap, (i - r0 + 1) cap) of
 * ids_dev / counts_dev: its qualifying columns in ASCENDING j with their counts -- bit-reproducible -- and rowcnt_dev[i - r0] is the
 * TRUE number even beyond cap; nothing is written past a row's slots (cap == 0: counting only, ids_dev / counts_dev may be NULL).
 * band_rows == 0: the default (a band of at most 64 MB).  Enqueues on `stream`, does not synchronise.  The band lives in the context:
 * the selection launches of ONE context must be issued on ONE stream.  The band only grows: a call that has to grow it (this one,
 * d2g_cmp_dedup_dev, d2g_edit_within_dev, d2g_edit_dedup_dev) waits for the device before it releases the old block (hipFree), so
 * calls queued earlier that still read that block finish first; such a call does synchronise, and it allocates. */
int  d2g_cmp_knn_dev(d2g_ctx *ctx, const d2g_cmp_set *set, size_t r0, size_t r1, size_t K, uint32_t min_count,
                     const uint32_t *cls_dev, size_t cap, uint32_t *rowcnt_dev /* [r1-r0] */, uint32_t *ids_dev /* [r1-r0][cap] */,
                     uint32_t *counts_dev /* [r1-r0][cap] */, size_t band_rows, void *stream);
/* Host half (no context): candidate lists -> CSR in the reference's order.  value = lut[count] (lut: sketchsize + 1 floats); inside a
 * row best value first -- descending (isdist == 0) or ascending (isdist != 0) -- and equal values by ascending id: std::sort of
 * (+-value, id), src/index_build.h:16; the values written are the plain lut entries.  indptr_out has nrows + 1 entries and is
 * always written; *nnz_needed (may be NULL) = the entries the lists hold; indices_out / data_out are written only when out_cap
 * holds them all, D2G_ERR_NOMEM otherwise.  A row with rowcnt > cap is INCOMPLETE: *overflow_rows (may be NULL) counts such rows, and
 * if there is one the call writes nothing else and returns D2G_ERR_INVALID (re-run those rows with a cap that fits); a count above
 * sketchsize is D2G_ERR_INVALID too.  Nothing is read past the first min(rowcnt, cap) slots of a row. */
int  d2g_knn_finish(const uint32_t *rowcnt, const uint32_t *ids, const uint32_t *counts, size_t nrows, size_t cap, const float *lut,
                    size_t sketchsize, int isdist, uint64_t *indptr_out /* [nrows+1] */, uint32_t *indices_out, float *data_out,
                    size_t out_cap, size_t *nnz_needed, size_t *overflow_rows);
/* Host-pointer form over a prepared set: exactly one of K >= 1 (top-K) and threshold > 0 ((double)value >= threshold, or <= for
 * isdist) selects the mode.  lut (host, sketchsize + 1 floats) must be monotone in the count -- non-decreasing for similarities,
 * non-increasing for distances (D2G_ERR_INVALID otherwise); in top-K mode with isdist == 0 a value of 0 is never a neighbour
 * (src/index_build.cpp:194).  Runs the rows in chunks with `cap` slots each (0 = a default from K), re-runs ONLY the rows whose
 * rowcnt exceeded cap with a cap that fits, finishes (d2g_knn_finish) and synchronises.  Outputs as d2g_knn_finish. */
int  d2g_cmp_set_knn(d2g_ctx *ctx, const d2g_cmp_set *set, size_t r0, size_t r1, const float *lut, int isdist, size_t K,
                     double threshold, size_t cap, size_t band_rows, uint64_t *indptr_out /* [r1-r0+1] */, uint32_t *indices_out,
                     float *data_out, size_t out_cap, size_t *nnz_needed);
/* ... and from the N x S matrix itself: upload, prepare, table (d2g_epilogue_lut: D2G_ERR_UNSUPPORTED where the value is not a
 * function of the equality count alone), d2g_cmp_set_knn.  isdist = the reference's distance(measure), src/cmp_main.h:44-49. */
int  d2g_cmp_knn(d2g_ctx *ctx, const uint64_t *sig_bits, size_t N, size_t sketchsize, size_t r0, size_t r1, int measure, int k,
                 int multiset_space, int algo, size_t K, double threshold, size_t cap, size_t band_rows,
                 uint64_t *indptr_out /* [r1-r0+1] */, uint32_t *indices_out, float *data_out, size_t out_cap, size_t *nnz_needed);

/* ---- K2f: greedy clustering on the device (cmp --greedy T) ---------------------------------------------------------------
 * Replaces the exhaustive branch of dedup_core (reference src/dedup_core.cpp:262-283) for values that are a NON-DECREASING function
 * of the equality count: in INPUT order, sketch i joins the representative with the largest value -- among equal values the one
 * with the smallest index -- if that value reaches the threshold, and founds a cluster otherwise.  A sketch is compared with
 * representatives only (A~B, B~C, A!~C gives {A,B},{C}).  Only assign[N] leaves the device.
 *
 * d2g_cmp_dedup_dev, any kind of set: a count c qualifies iff cls[c] >= min_count, "largest value" is the largest cls[c].
 *   cls_dev (NULL = identity) = S + 1 words, cls[e] = the smallest count whose VALUE equals that of e (so cls[e] <= e);
 *   min_count = the smallest count whose value reaches the threshold (S + 1: nobody ever joins).
 *   assign_dev[i] = the representative of i's cluster (i itself for a representative); every word of [0, N) is written, nothing else.
 * Rows are taken in bands of band_rows (0 = a default; at most 256, larger requests are cut to that: the in-order step is
 * sequential in the band) whose counts go into scratch of the context.  Enqueues on `stream`, does not synchronise; the calls of
 * ONE context that use the scratch band (this and d2g_cmp_knn_dev) must be issued on ONE stream.  N = 0 does nothing. */
int  d2g_cmp_dedup_dev(d2g_ctx *ctx, const d2g_cmp_set *set, uint32_t min_count, const uint32_t *cls_dev /* [S+1] or NULL */,
                       uint32_t *assign_dev /* [N] */, size_t band_rows, void *stream);
/* Host half (no context): assign -> clusters in creation order (= ascending representative), inside a cluster the representative
 * first, then its members in input order (dedup_emit's ids / constituents, src/dedup_core.cpp:400-451).  indptr_out has room for
 * N + 1 entries, of which *nclusters + 1 are written; indices_out has N.  D2G_ERR_INVALID (nothing promised about the outputs) if
 * assign[i] > i or assign[assign[i]] != assign[i]. */
int  d2g_dedup_clusters(const uint32_t *assign, size_t N, uint64_t *indptr_out, uint32_t *indices_out /* [N] */, size_t *nclusters);
/* Host-pointer form over a prepared set.  lut (host, sketchsize + 1 floats) must be non-decreasing (D2G_ERR_INVALID otherwise);
 * simt = (float)(threshold > 0 ? threshold : 0.9), i joins iff !(value < simt) in float (dedup_core.cpp:264,276).  Runs the whole
 * set, copies back 4 N bytes and synchronises. */
int  d2g_cmp_set_dedup(d2g_ctx *ctx, const d2g_cmp_set *set, const float *lut, double threshold, size_t band_rows,
                       uint32_t *assign_out /* host [N] */);
/* ... and from the N x S matrix itself.  D2G_ERR_UNSUPPORTED where d2g_epilogue_lut fails, or for a distance (D2G_POISSON_LLR): with
 * one the reference's test founds a new cluster exactly when the nearest representative is CLOSER than the threshold. */
int  d2g_cmp_dedup(d2g_ctx *ctx, const uint64_t *sig_bits, size_t N, size_t sketchsize, int measure, int k, int multiset_space,
                   int algo, double threshold, size_t band_rows, uint32_t *assign_out /* host [N] */);

/* ---- multi-GPU: RCCL communicator + row-sharded all-pairs engine ------------------------------------
 * Replaces nothing in the reference (it has no multi-process code); it is how the all-pairs seam
 * (cmp_core -> emit_rectangular, src/cmp_core.cpp:746-751) spreads over the GPUs of a node: rows of the upper
 * triangle are independent units, one exchange of the compact bit-plane operand, no reduction.
 * One d2g_ctx + one d2g_comm + one d2g_allpairs per GPU.  Two deployments share all of it:
 *   - one process (or host thread) per GPU: rank 0 calls d2g_comm_unique_id, the 128 bytes reach the other
 *     ranks by any means (file, socket, MPI, a torch.distributed store), every rank calls d2g_comm_create;
 *   - one process driving several GPUs (the `dashing2 cmp` CLI): d2g_comm_create_all + the `_all` entry
 *     points, which issue each collective phase for all ranks inside one RCCL group.
 * RCCL is loaded at first use (dlopen); contexts that share a device get a loopback transport instead
 * (device copies ordered by events; D2G_COMM_LOOPBACK=1 asks for it over distinct devices too) so that the whole
 * path can be exercised on one GPU.  The ranks of a loopback group are driven together through the `_all` entry
 * points, each rank exactly once per call: a per-rank entry point
 * (d2g_allpairs_prepare_dev / _step_*_dev / _enqueue_lut_dev) on such a group returns D2G_ERR_INVALID before it
 * enqueues anything (it could never meet its peers' transfers), and the group stays usable.
 * An engine allocates on first use: its operand buffers at create (the second one in the first pipelined call), a
 * rank's exporter sets in its first prepare.  Each of these zeroes its buffers on the null stream and waits for that
 * on the host (hipStreamSynchronize(NULL)) before it returns, so that work on a non-blocking stream cannot overtake
 * the zeroing: the first prepare / first pipelined call of an engine blocks the host briefly, later ones do not. */
typedef struct d2g_comm d2g_comm;
#define D2G_COMM_ID_BYTES 128
int  d2g_comm_unique_id(void *id_out /* D2G_COMM_ID_BYTES */);                       /* ncclGetUniqueId */
int  d2g_comm_create(d2g_ctx *ctx, const void *id, int rank, int world, d2g_comm **out);   /* ncclCommInitRank (collective) */
int  d2g_comm_create_all(d2g_ctx **ctxs, int nctx, d2g_comm **comms_out /* [nctx] */);     /* ncclCommInitAll, or loopback */
void d2g_comm_destroy(d2g_comm *comm);
int  d2g_comm_rank(const d2g_comm *comm);
int  d2g_comm_world(const d2g_comm *comm);
int  d2g_comm_is_rccl(const d2g_comm *comm);                                          /* 0: loopback / single rank without id */
/* the host matrix to every GPU of this process -- one H2D to ctxs[0], then one RCCL
 * broadcast over xGMI.  sig_dev_out[i] is allocated on ctxs[i] (release with d2g_free).  Synchronises. */
int  d2g_bcast_sigs(d2g_ctx **ctxs, d2g_comm **comms, int nctx, const uint64_t *host_sig, size_t N, size_t sketchsize,
                    uint64_t **sig_dev_out /* [nctx] */);

typedef struct d2g_allpairs d2g_allpairs;
/* rank `d2g_comm_rank(comm)` of an all-pairs job over an N x S matrix.  No divisibility requirement on N or S. */
int  d2g_allpairs_create(d2g_ctx *ctx, d2g_comm *comm, size_t N, size_t sketchsize, d2g_allpairs **out);
void d2g_allpairs_destroy(d2g_allpairs *eng);
/* rows [lo, hi) of the matrix this rank must HOLD as its input block (contiguous, sizes differ by <= 1) */
int  d2g_allpairs_rows_held(const d2g_allpairs *eng, size_t *lo, size_t *hi);
/* rows [r0, r1) of the upper triangle this rank COMPUTES (pair-balanced, d2g_ut_partition) */
int  d2g_allpairs_rows_computed(const d2g_allpairs *eng, size_t *r0, size_t *r1);
/* exchange + sharded prepare: afterwards d2g_allpairs_operand() is the whole N x S bit-sliced operand on this
 * rank's GPU, usable with d2g_cmp_eqcount_ut_dev / d2g_cmp_lut_ut_dev / d2g_cmp_eqcount_rect_dev on ANY rows
 * (the CLI deals row batches to the GPUs round-robin).  Collective; enqueues on `stream`, no synchronisation. */
int  d2g_allpairs_prepare_dev(d2g_allpairs *eng, const uint64_t *my_rows_dev /* [hi-lo][S] */, void *stream);
int  d2g_allpairs_prepare_all(d2g_allpairs **engs, int n, const uint64_t *const *rows_dev, void *const *streams);
const d2g_cmp_set *d2g_allpairs_operand(const d2g_allpairs *eng);
/* The sharded prepare can fail for the reason d2g_cmp_set_status documents (rank-table overflow on an adversarial column), on
 * ANY rank; every rank's status word travels with its groups, so each rank learns it.  Synchronises `stream`; D2G_ERR_INTERNAL
 * means the results of the last prepare/step are invalid on every rank (fall back to one GPU with D2G_CMP_DIRECT).
 * d2g_cmp_set_status(d2g_allpairs_operand(eng)) returns the same. */
int  d2g_allpairs_status(d2g_allpairs *eng, void *stream);
/* chunks the engine cuts a rank's column slice into: the exchange of chunk c+1 overlaps the prepare of chunk c inside ONE step
 * (a function of N, S and the world size; D2G_MGPU_CHUNKS overrides it -- identically on every rank: with one process per GPU
 * d2g_allpairs_create exchanges (N, S, world, chunks) over the communicator once and fails with D2G_ERR_INVALID on every rank
 * when any two ranks disagree, instead of posting mismatched transfers later) */
int  d2g_allpairs_chunks(const d2g_allpairs *eng);
/* one whole step: prepare + this rank's slab (rows_computed) of the condensed triangle; out has
 * d2g_ut_count(N, r0, r1) entries.  lut_dev == NULL (or lut_dev[i] == NULL): u32 equality counts. */
int  d2g_allpairs_step_lut_dev(d2g_allpairs *eng, const uint64_t *my_rows_dev, const float *lut_dev, float *out_dev, void *stream);
int  d2g_allpairs_step_eqcount_dev(d2g_allpairs *eng, const uint64_t *my_rows_dev, uint32_t *out_dev, void *stream);
int  d2g_allpairs_step_all(d2g_allpairs **engs, int n, const uint64_t *const *rows_dev, const float *const *lut_dev,
                           void *const *out_dev, void *const *streams);
/* Per-phase times of ONE step (what a scaling run needs to check a cost model term by term).  With phase timing on, every phase
 * the next prepare/step enqueues for this engine is bracketed by timing events on the stream it runs on (a few microseconds
 * each: switch it off for timed runs); d2g_allpairs_phase_times synchronises the device and returns one record per phase in
 * enqueue order: kind (D2G_PHASE_*), chunk, start (ms after the step's first enqueue reached the GPU) and duration (ms).
 * An exchange phase's duration includes waiting for the slowest peer. */
#define D2G_PHASE_PACK    0
#define D2G_PHASE_X1      1   /* rows -> column slices ("all-to-all-v"), per chunk */
#define D2G_PHASE_PREPARE 2   /* transpose + rank + plan + planes of this rank's column chunk */
#define D2G_PHASE_X2      3   /* bit-plane groups to everyone ("all-gather-v"), per chunk */
#define D2G_PHASE_DERIVE  4   /* plane stream of a gathered chunk */
#define D2G_PHASE_PAIR    5   /* the pair kernel over this rank's rows (d2g_allpairs_step_* only) */
#define D2G_PHASE_ORDER   6   /* sparse tiles on the gathered operand (N >= 8192): ids from the planes, sketch order, sorted stream */
#define D2G_PHASE_FILL    7   /* the slab pre-filled with the value of "0 equal" at the start of the step, under the exchanges (sparse path) */
int  d2g_allpairs_set_phase_timing(d2g_allpairs *eng, int on);
int  d2g_allpairs_phase_times(d2g_allpairs *eng, int cap, int *n_out, int *kind /* [cap] */, int *chunk /* [cap] */,
                              float *start_ms /* [cap] */, float *dur_ms /* [cap] */);
/* what the sparse-tile path did in this engine's LAST pair phase (device-synchronising): info4 as d2g_cmp_set_sparse_info --
 * [0] the gathered operand was ordered (N >= 8192), [1] tiles listed, [2] bit 0 dense walk decided by the ordering / bit 1 the dense kernel ran /
 * bit 2 tiles + pair list used / bit 3 the gathered order was kept, [3] entries of the pair list. */
int  d2g_allpairs_sparse_info(d2g_allpairs *eng, uint32_t *info4);
/* software-pipelined step for a stream of matrices: the exchange + prepare of this call overlap the pair kernel
 * of the previous call (own stream, two operand buffers); results land in out_dev in call order on `stream`.
 * input_ready != 0: my_rows_dev is already complete (no dependency on work queued on `stream`).
 * Plain (prepare/step) and pipelined calls may be mixed on one engine: each form waits, through events, for what the
 * other still has in flight on the buffers they share. */
int  d2g_allpairs_enqueue_lut_dev(d2g_allpairs *eng, const uint64_t *my_rows_dev, const float *lut_dev, float *out_dev,
                                  void *stream, int input_ready);

/* ---- K3s + K2g: exact k-mer sets, --set and --countdict (reference src/counter.h:78-117, src/fastxsketch.cpp:425-524,
 * src/wcompare.cpp:145-187, src/cmp_core.cpp:518-575) ----------------------------------------------------------------
 * E_g = the pairs (h, c) of every DISTINCT masked k-mer h = maskfn(kmer) of input g and its number of occurrences c, kept iff
 * c > count_threshold (the Counter's convention, src/counter.h:87), ascending by h.  d2g_kmer_sets is d2g_kmer_count WITH the
 * reference's sort, done on the device: set g = keys_out / counts_out [set_off_out[g], set_off_out[g+1]), strictly ascending keys;
 * counts_out may be NULL (keys only).  cards_out [n][2]: cards_out[2g] = |E_g| (the cardinality under --set), cards_out[2g+1] = the
 * integer sum of E_g's counts (under --countdict, src/fastxsketch.cpp:441).  cap = capacity of keys_out and counts_out in entries
 * (the total k-mer count always suffices); a cap that is too small is D2G_ERR_INVALID with a message that names the need, and
 * NOTHING is written to any output.  The _dev form takes device pointers, honours the plan's k-mer filter and synchronises
 * `stream` (twice: for the total, and for the status word of the kernels), like d2g_bmh_sketch_dev. */
int d2g_kmer_sets(d2g_ctx *ctx, const uint8_t *packed, size_t packed_bytes,
                  const uint64_t *run_start, const uint32_t *run_len, size_t nrun,
                  const uint64_t *genome_run_off, size_t n, int k, int canon, uint64_t xormask,
                  double count_threshold, uint64_t *keys_out, uint32_t *counts_out /* or NULL */, size_t cap,
                  uint64_t *set_off_out /* [n+1] */, uint64_t *cards_out /* [n][2] */);
/* persistent form (same buffers/stream as d2g_sketcher_run; honours the sketcher's k-mer filter) */
int d2g_sketcher_run_sets(d2g_sketcher *sk, const uint8_t *packed, size_t packed_bytes,
                          const uint64_t *run_start, const uint32_t *run_len, size_t nrun,
                          const uint64_t *genome_run_off, size_t n, int k, int canon, uint64_t xormask,
                          double count_threshold, uint64_t *keys_out, uint32_t *counts_out /* or NULL */, size_t cap,
                          uint64_t *set_off_out /* [n+1] */, uint64_t *cards_out /* [n][2] */);
int d2g_kmer_sets_dev(d2g_ctx *ctx, const d2g_oph_plan *plan, const uint8_t *packed_dev, int canon, uint64_t xormask,
                      double count_threshold, uint64_t *keys_dev, uint32_t *counts_dev /* or NULL */, size_t cap,
                      uint64_t *set_off_dev /* [n+1] */, uint64_t *cards_dev /* [n][2] */, void *stream);
/* A d2g_kset owns N such sets in device memory (keys, optional counts, offsets) and a table that cuts every set at the same 2^p
 * key values.  isz(i, j) = sum over the keys both sets hold of min(w_i, w_j), w = 1 without counts, = the count with them: an
 * integer, returned exactly as u64.  There is no floating point on the device path.
 * d2g_kset_check: the host-side check of d2g_kset_create on its own (no context, no device): D2G_ERR_INVALID with a message in
 * err (may be NULL) for a set_off that is not monotone and for a set whose keys are not STRICTLY ascending (unsorted, duplicate);
 * with counts, for a count of 0.
 * d2g_kset_create copies host arrays (loaded files) after that check; it refuses with D2G_ERR_NOMEM and a message that names the bytes
 * needed and the bytes free when the sets do not fit in device memory (there is no out-of-core path).
 * d2g_kset_create_dev copies the device arrays d2g_kmer_sets_dev produced (set_off_dev is read once, after `stream` is waited for;
 * the arrays are the caller's to free afterwards).  It trusts their order. */
typedef struct d2g_kset d2g_kset;
int    d2g_kset_check(const uint64_t *keys, const uint32_t *counts /* or NULL */, const uint64_t *set_off /* [nsets+1] */, size_t nsets,
                      char *err, size_t errcap);
int    d2g_kset_create(d2g_ctx *ctx, const uint64_t *keys, const uint32_t *counts /* or NULL */, const uint64_t *set_off /* [nsets+1] */,
                       size_t nsets, d2g_kset **out);
int    d2g_kset_create_dev(d2g_ctx *ctx, const uint64_t *keys_dev, const uint32_t *counts_dev /* or NULL */, const uint64_t *set_off_dev,
                           size_t nsets, void *stream, d2g_kset **out);
void   d2g_kset_destroy(d2g_kset *ks);
size_t d2g_kset_size(const d2g_kset *ks);                    /* N */
size_t d2g_kset_device_bytes(const d2g_kset *ks);            /* resident bytes: keys, counts, offsets, slice table */
int    d2g_kset_slice_bits(const d2g_kset *ks);              /* p */
/* rows [r0, r1) of the condensed upper triangle, in the order of d2g_cmp_eqcount_ut_dev: d2g_ut_count(N, r0, r1) u64 */
int    d2g_kset_isz_ut_dev(d2g_ctx *ctx, const d2g_kset *ks, size_t r0, size_t r1, uint64_t *out_dev, void *stream);
/* the row-major block rows [a0, a1) x columns [b0, b1), isz(row, column) (--square, -Q) */
int    d2g_kset_isz_rect_dev(d2g_ctx *ctx, const d2g_kset *ks, size_t a0, size_t a1, size_t b0, size_t b1, uint64_t *out_dev, void *stream);
/* the exact branch of compare(), src/cmp_core.cpp:518-575 (CORRECT_RES), in double, then the cast to float: with res = (double)isz,
 * SIMILARITY res / (lhcard + rhcard - res); POISSON_LLR (--mash-distance) sim2dist of that; CONTAINMENT res / lhcard;
 * SYMMETRIC_CONTAINMENT res / min(lhcard, rhcard); INTERSECTION res; UNION_SIZE lhcard + rhcard - res (the reference has no arm for
 * it and returns res: not reproduced).  NaN or Inf becomes the maximum (:573-575): two empty inputs take that route. */
float  d2g_epilogue_exact(uint64_t isz, double lhcard, double rhcard, int measure, int k);
int    d2g_epilogue_exact_ut(const uint64_t *isz, const double *cards, size_t N, size_t r0, size_t r1, int measure, int k, int nthreads,
                             float *out);
int    d2g_epilogue_exact_rect(const uint64_t *isz, const double *cards, size_t N, size_t a0, size_t a1, size_t b0, size_t b1,
                               int measure, int k, int nthreads, float *out);

/* ---- K2h: exact edit distances between records, --parse-by-seq --edit-distance --compute-edit-distance (reference
 * src/cmp_core.cpp:331-347,450-457: edlibAlign in global distance mode on the two records' raw bytes) ---------------------
 * d(i, j) = the unit-cost Levenshtein distance between the BYTES of records i and j: no case folding, every byte value its own
 * symbol.  An integer, returned exactly as u32.  There is no floating point on the device path.
 *
 * d2g_seqrecs: the host record reader.  The kseq record walk of d2g_seqpack_add_path_by_record / _add_fastx_by_record (the same
 * walker: names and record boundaries cannot differ), keeping the raw sequence bytes instead of packing them: names, one
 * concatenated byte array, off[n + 1].  An empty record is kept with length 0.  A record that the walk drops as an error (a FASTQ
 * record whose quality length differs) is dropped here too, and ends the input. */
typedef struct d2g_seqrecs d2g_seqrecs;
int             d2g_seqrecs_create(d2g_seqrecs **out);
void            d2g_seqrecs_destroy(d2g_seqrecs *sr);
int             d2g_seqrecs_add_path(d2g_seqrecs *sr, const char *path_line);   /* FASTA/FASTQ(.gz), space-separated sub-paths */
int             d2g_seqrecs_add_fastx(d2g_seqrecs *sr, const char *buf, size_t len);
size_t          d2g_seqrecs_nrecords(const d2g_seqrecs *sr);
const char     *d2g_seqrecs_name(const d2g_seqrecs *sr, size_t record);
const uint8_t  *d2g_seqrecs_bytes(const d2g_seqrecs *sr);
const uint64_t *d2g_seqrecs_off(const d2g_seqrecs *sr);              /* [nrecords + 1] */
/* A d2g_seqset owns N records in device memory, recoded to dense codes 0 .. sigma - 1 in order of byte value (sigma = the number of
 * distinct byte values of the set, 1 <= sigma <= 256; a set without a byte has sigma = 1), each record padded to 16 codes, with
 * their lengths and an order of the records by length.
 * d2g_seqset_check: the host-side check of d2g_seqset_create on its own (no context, no device): D2G_ERR_INVALID with a message in
 * err (may be NULL) for null tables, an off that does not begin at 0 or decreases, off[nrec] != nbytes; D2G_ERR_UNSUPPORTED for a
 * record of more than D2G_EDIT_MAX_LEN symbols (the message has the record and its length).
 * d2g_seqset_recode_map: map[b] = the code of byte value b (0 for a value that does not occur); returns sigma.
 * d2g_seqset_create copies the records once and recodes them on the device; D2G_ERR_NOMEM with the bytes needed and the bytes free
 * when they do not fit, never a smaller object. */
#define D2G_EDIT_MAX_LEN 65535
typedef struct d2g_seqset d2g_seqset;
int    d2g_seqset_check(const uint8_t *bytes, const uint64_t *off /* [nrec+1] */, size_t nrec, uint64_t nbytes, char *err, size_t errcap);
int    d2g_seqset_recode_map(const uint8_t *bytes, uint64_t nbytes, uint8_t map[256]);
int    d2g_seqset_create(d2g_ctx *ctx, const uint8_t *bytes, const uint64_t *off /* [nrec+1] */, size_t nrec, uint64_t nbytes, d2g_seqset **out);
void   d2g_seqset_destroy(d2g_seqset *ss);
size_t d2g_seqset_nrecords(const d2g_seqset *ss);
size_t d2g_seqset_device_bytes(const d2g_seqset *ss);        /* resident bytes: codes, offsets, lengths, order */
int    d2g_seqset_alphabet_size(const d2g_seqset *ss);       /* sigma */
/* the 32-row blocks of a query that one strip of the pair kernel holds for this set under this context's switches (D2G_EDIT_STRIP):
 * a longer query runs strip by strip */
int    d2g_seqset_strip_blocks(const d2g_ctx *ctx, const d2g_seqset *ss);
/* rows [r0, r1) of the condensed upper triangle, in the order of d2g_kset_isz_ut_dev: d2g_ut_count(N, r0, r1) u32.  A pair with an
 * empty record yields the other's length.  An empty range is D2G_OK and writes nothing; a set of another context is D2G_ERR_INVALID
 * before anything is written. */
int    d2g_edit_ut_dev(d2g_ctx *ctx, const d2g_seqset *ss, size_t r0, size_t r1, uint32_t *out_dev, void *stream);
/* the row-major block rows [a0, a1) x columns [b0, b1), d(row, column); (r, r) is 0 (--square) */
int    d2g_edit_rect_dev(d2g_ctx *ctx, const d2g_seqset *ss, size_t a0, size_t a1, size_t b0, size_t b1, uint32_t *out_dev, void *stream);
/* host-pointer forms; synchronise */
int    d2g_edit_ut(d2g_ctx *ctx, const d2g_seqset *ss, size_t r0, size_t r1, uint32_t *out);
int    d2g_edit_rect(d2g_ctx *ctx, const d2g_seqset *ss, size_t a0, size_t a1, size_t b0, size_t b1, uint32_t *out);

/* ---- K2i: neighbours within a bound on the edit distance (reference src/index_build.cpp:166-228, build_exact_graph with
 * M_EDIT_DISTANCE as the distance) -----------------------------------------------------------------------------------------
 * For a bound T >= 0 the CLOSENESS of records i and j is c(i, j) = T + 1 - d(i, j) if d(i, j) <= T, else 0, with d the distance of
 * K2h above: c = T + 1 - min(d, T + 1), an exact integer in [0, T + 1]; c(i, i) = T + 1.  Larger is nearer and 0 is never a
 * neighbour, so closeness is to K2e's selection what the equality count is (S = T + 1).  No floating point on the device.
 *
 * d2g_edit_near_dev writes c(i, j) for every row i in [r0, r1) and EVERY column j in [0, N), row-major; nothing is left unwritten.
 * T < 2^31.  Per pair: |len_i - len_j| > T gives 0 without a table (the columns that can pass are one window of the set's order by
 * length; the rest is a fill); for T <= D2G_EDIT_BAND_MAX a kernel that gives every LANE one column record and slides the band of
 * 2T + 1 diagonals down the query in one 64-bit word, leaving a pair as soon as its score proves d > T; above that bound (and for a
 * row whose match table would not fit in 64 KiB of LDS: (ceil(len / 32) + 4 | 1) * sigma > 16384; and for a row of 9 to 32 symbols
 * with 5T >= its length, where that kernel was measured to be ahead) the pair kernel of K2h over the
 * window, into close_dev itself, then a clamp in place.  The route is chosen per row and [r0, r1) is cut into runs of CONSECUTIVE rows of
 * one route, a launch (or two) each: rows that alternate between the routes cost a launch per row (not measured; a set of one kind of
 * record, or one sorted by length, has at most three runs).  Enqueues on `stream`, does not synchronise, allocates nothing.  An empty
 * row range is D2G_OK and writes nothing; a set of another context or a null output is D2G_ERR_INVALID before anything is written. */
#define D2G_EDIT_BAND_MAX 31
int    d2g_edit_band_max(void);                              /* D2G_EDIT_BAND_MAX of the library that was loaded */
int    d2g_edit_near_dev(d2g_ctx *ctx, const d2g_seqset *ss, size_t r0, size_t r1, uint32_t T, uint32_t *close_dev /* [r1-r0][N] */,
                         void *stream);
/* The selection of d2g_cmp_knn_dev (K2e, the same kernel) over closeness, with min_count = 1 and cls = NULL: per row of [r0, r1) the
 * columns j != i (self excluded by INDEX: duplicates list each other) in ASCENDING j with their closeness in the row's own cap slots,
 * rowcnt_dev the TRUE number even beyond cap, nothing written past a row's slots; cap == 0 counts only (ids_dev / close_dev may be
 * NULL).  K == 0: every j with d <= T.  K >= 1: the K nearest among those with d <= T with all ties of the K-th; a row with fewer
 * than K inside the bound lists what it has.  Bands of band_rows rows (0 = a default) go through the context's ONE scratch band, the
 * one d2g_cmp_knn_dev and d2g_cmp_dedup_dev use: the calls of one context that use it must be issued on ONE stream.  Enqueues, does
 * not synchronise. */
int    d2g_edit_within_dev(d2g_ctx *ctx, const d2g_seqset *ss, size_t r0, size_t r1, size_t K, uint32_t T, size_t cap,
                           uint32_t *rowcnt_dev /* [r1-r0] */, uint32_t *ids_dev /* [r1-r0][cap] */, uint32_t *close_dev /* [r1-r0][cap] */,
                           size_t band_rows, void *stream);
/* Host-pointer form, in the manner of d2g_cmp_set_knn: rows in chunks with `cap` slots each (0 = a default), only the rows that
 * overflowed cap run again, d2g_knn_finish with lut[c] = (float)(T + 1 - c), isdist = 1; synchronises.  The values are the distances
 * as float32, ascending, equal distances by ascending id (std::sort of (value, id)).  Outputs and errors as d2g_cmp_set_knn:
 * indptr_out [r1 - r0 + 1] is always written, D2G_ERR_NOMEM with *nnz_needed when out_cap is short, D2G_ERR_INVALID for a bad range.
 * As there, the whole result is computed before out_cap is looked at: a caller that retries after D2G_ERR_NOMEM pays the device work
 * twice (pass an out_cap that is large enough where a bound on nnz is known).
 *   K == 0, threshold mode: every j != i with d(i, j) <= T (the NN_GRAPH_THRESHOLD arm for a distance; a caller with a non-integer
 *           threshold passes its floor).
 *   K >= 1, top-K mode: the K smallest distances over ALL other records with every tie of the K-th, no zero-skipping.
 *           T is only the STARTING bound: the rows that end with fewer than min(K, N - 1) entries, and only those, run again with
 *           the bound 2T + 1, until they are full or the bound reaches the set's longest record, from where every record
 *           qualifies.  The result does not depend on T. */
int    d2g_edit_knn(d2g_ctx *ctx, const d2g_seqset *ss, size_t r0, size_t r1, size_t K, uint32_t T, size_t cap, size_t band_rows,
                    uint64_t *indptr_out /* [r1-r0+1] */, uint32_t *indices_out, float *data_out, size_t out_cap, size_t *nnz_needed);

/* ---- K2j: greedy clustering by edit distance (the repository's own rule; the reference's exhaustive dedup_core is
 * inverted for a distance, SURVEY F13, and is not reproduced) ---------------------------------------------------------------
 * Records are taken in input order i = 0 .. N - 1; d is the distance of K2h above (unit costs, bytes as they are, d(x, "") = |x|).
 * Among the representatives r < i the one with the smallest d(i, r) is picked, among equal distances the smallest r; if that
 * distance is <= T, assign[i] = r, otherwise i is a representative and assign[i] = i.  A record is compared with representatives
 * only: A ~ B, B ~ C, A !~ C gives {A, B}, {C}.  In the closeness c = T + 1 - min(d, T + 1) of K2i this is the rule of
 * d2g_cmp_dedup_dev with the identity class table and min_count = 1, and d2g_dedup_clusters turns assign into clusters unchanged.
 *
 * d2g_edit_dedup_dev writes every word of assign_dev[0, N) and nothing else of the caller's.  It enqueues on `stream` and never
 * synchronises with the host (the length of the representative list stays in a device word).  Bands of band_rows rows (0 = the
 * default, 256; larger requests are cut to 256, as in d2g_cmp_dedup_dev).  For T <= D2G_EDIT_BAND_MAX a row whose match table fits in
 * 64 KiB of LDS ((ceil(len / 32) + 4 | 1) * sigma <= 16384) runs the band kernel of K2i over the list of representatives in front of
 * its band and keeps only the best key per row; every other row runs d2g_edit_near_dev over all N columns into the context's scratch
 * band.  It may GROW scratch of the context (the band of d2g_edit_within_dev / d2g_cmp_knn_dev / d2g_cmp_dedup_dev, K2f's keys, and a
 * list of N + 66 561 words of its own): the calls of one context that use that scratch must be issued on ONE stream.  T < 2^31 - 1.
 * N = 0 does nothing and is D2G_OK.  A set of another context, or a null output, is D2G_ERR_INVALID before anything is written; a
 * null context or set returns D2G_ERR_INVALID (-1) without a message.
 * d2g_edit_dedup runs the set, copies the 4 N bytes of assign to assign_out and synchronises. */
int    d2g_edit_dedup_dev(d2g_ctx *ctx, const d2g_seqset *ss, uint32_t T, uint32_t *assign_dev /* [N] */, size_t band_rows, void *stream);
int    d2g_edit_dedup(d2g_ctx *ctx, const d2g_seqset *ss, uint32_t T, size_t band_rows, uint32_t *assign_out /* host [N] */);

/* ---- multi-GPU row partition (host arithmetic; emitrect.cpp:290-323 row order) ----
 * Splits rows [0,N) into `nparts` contiguous ranges with (near-)equal pair counts.
 * bounds_out has nparts+1 entries. */
int  d2g_ut_partition(size_t N, int nparts, size_t *bounds_out);

#ifdef __cplusplus
}
#endif
#endif
