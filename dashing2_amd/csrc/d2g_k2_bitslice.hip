// d2g_k2_bitslice.hip -- K2, BITSLICE algorithm (gfx950): exact equality counts from bit planes.
//
// Same contract as the direct kernel (reference src/cmp_core.cpp:461,506 count_gtlt/count_eq
// inside src/emitrect.cpp:211-323), different arithmetic:
//
//   the count only needs EQUALITY of 64-bit patterns within one register index t, so each
//   column t of the N x S matrix is first mapped to small ids: a value that occurs >= 2 times in its
//   column gets a dense rank 1..D2; a value that occurs once can never equal anything ("unique").
//   The ids are stored bit-sliced, in TWO codings of the unique values: the ROW operand codes them
//   as 0, the COLUMN operand as all-ones (2^nbits - 1 > D2), so a unique value mismatches whatever
//   it meets without a separate test.  Word P[tb][b][j] holds bit b of the ids of sketch j for the
//   32 registers t = 32*tb .. 32*tb+31.  For a pair (i,j) and a 32-register group
//       z = OR_b ( R[tb][b][i] XOR C[tb][b][j] )          one v_bitop3_b32 per plane
//       mismatches += popcount(z)                          one v_bcnt_u32_b32 (accumulating)
//   i.e. (nbits+1)/32 VALU operations per register compare instead of 2 (v_cmp_eq_u64+v_addc):
//   0.25 at 7 planes.  Row operands come through SCALAR loads (one s_load_dwordx16 per plane
//   serves 16 rows), column operands are one coalesced dword per lane.
//
// Prepare = 3 small kernels (timed as "k2prep"): transpose, per-column open-addressing insert into an
// LDS owner table + compaction to dense ranks, 32 x nbits bit transpose into both codings.
#include "d2g_internal.h"
#include "d2g_k2.h"
#include "d2g_k2_shape.h"
#include <chrono>
#include <cstring>
#include <algorithm>
#include <vector>

namespace {

typedef uint32_t u32x16 __attribute__((ext_vector_type(16)));
typedef u32x16 __attribute__((aligned(4))) u32x16_u;
constexpr uint32_t BS_EMPTY = 0xFFFFFFFFu;

// ------------------------------------------------------------------ 1. per-column dense ids
// One workgroup per register index t.  owner[] (T slots, pre-set to EMPTY) records the first
// sketch index that claimed a slot; equality is decided against that sketch's value, so no key
// storage and no reserved sentinel value is needed.
constexpr uint32_t BS_DUP = 0x80000000u;       // owner-table flag: the value has been seen again
constexpr uint32_t BS_UNIQ = 0x80000000u;      // id flag: value occurs once in its column (never equal)
constexpr uint32_t BS_PENDING = 0x40000000u;   // multi-partition rank kernel: ids[] holds a table slot of the current pass
constexpr int BS_LOG_TLDS_MAX = 15;            // LDS owner table: at most 32768 slots = 128 KiB
// The width of an id word is a property of the SET (d2g_cmp_set::id_bits).  A set ranked by a single-partition kernel (N <= 21 845: FAST or general) holds, per
// (column, sketch), 0 = padding, the unique flag, or a plain rank 1 .. D2 with D2 <= N / 2 <= 10 922: 16 bits carry that -- 0x8000 = unique, 1 .. 0x7FFF = rank --
// and every pass over ids[] moves half the bytes (D2G_BS_ID16=0: 32-bit words everywhere).  BS_PENDING and the split tag of bits 28-29 exist in the MULTI
// kernel only; MULTI, split and unpacked (sp_unpack_kernel) sets keep 32-bit words.  Every kernel that touches ids takes the word type as a template parameter.
template <typename IdT> struct BsId;
template <> struct BsId<uint32_t> { static constexpr uint32_t UNIQ = BS_UNIQ; static constexpr int UBIT = 31; };
template <> struct BsId<uint16_t> { static constexpr uint32_t UNIQ = 0x8000u; static constexpr int UBIT = 15; };
constexpr size_t BS_ID16_MAX_N = ((size_t(1) << BS_LOG_TLDS_MAX) * 2) / 3;      // = 21 845: the largest N whose hash space (>= 1.5 N slots) is one LDS table
static_assert(BS_ID16_MAX_N / 2 < BsId<uint16_t>::UNIQ, "16-bit ids: the highest rank (N / 2) must stay below the unique flag");
static_assert((size_t(1) << BS_LOG_TLDS_MAX) - 1 <= 0xFFFFu, "16-bit ids: the general single-partition kernel parks a table slot in ids[] between its two loops");

__device__ __forceinline__ uint32_t bs_hash(uint64_t v, int logT) {
    // Fibonacci hashing: the top logT bits of the product (partition = top bits, slot = low bits of those)
    return (uint32_t)((v * 0x9E3779B97F4A7C15ull) >> (64 - logT));
}

// Singleton folding: a value that occurs exactly once in its register column can never compare
// equal to anything, so all such values share id 0 and set the "unique" bit instead; only values
// occurring >= 2 times get dense ids 1..D2.  meta[t/32] = max over the group's columns of D2 + 1.
//
// One workgroup per register index t.  The T-slot hash space is walked in P = T / Tl partitions
// (top hash bits); each pass inserts the values of one partition into a Tl-slot LDS table of
// *owner sketch indices* (equality is decided against the owner's value: no key storage, no
// reserved sentinel), compacts the slots whose value was seen again into dense ranks, and
// writes the ids of that partition.  T >= 1.5 N, so a partition holds <= 2/3 Tl values on average.
// MULTI: more than one partition (N > 21845).  FAST: one partition and N <= 12288 -- a thread keeps all its values in
// registers; a kernel of its own so that the general path's registers do not cost it the second workgroup per CU.
// SPLIT (MULTI only): `nsplit` workgroups share one column, workgroup h = blockIdx.x / S walks the partitions
// [h nparts/nsplit, (h+1) nparts/nsplit) and ranks its values from 1 on its own; the ids carry h in bits 28-29 and
// bs_planes_kernel adds the offset of split h (the shared values the splits before it found: colcnt[t][h] after
// bs_colplan_kernel).  A column slice of N = 50 000 sketches x 64 registers -- one chunk of one rank of the 8-GPU
// exchange -- is 64 workgroups of one per CU otherwise: a quarter of the chip.
// (Measured in round 5 and dropped: a MULTI kernel that reads the column ONCE -- a thread keeps the high word of v * K of its <= 49 values
// in registers, every partition pass claims / confirms / ranks from them and writes final ids, no pending words -- for N <= 50 176.
// 128 VGPRs with ~320 spills, and the confirm step still fetches one owner value per candidate, four candidates in flight per thread:
// 2.58 ms instead of 1.04 at N = 50 000, 1.00 instead of 0.36 at N = 30 000.  What bounds this kernel at that size is not the repeated
// column read but the ~N gathers of 8 bytes per column that decide equality against the owner's value (51 million 64-byte sectors).
// Also measured and dropped: the values of a pass's partition COMPACTED into a queue in the LDS behind the table (block scan of the
// per-thread counts, 2560 entries of (value, sketch)) so that claim / confirm run with every lane busy instead of under an execution
// mask -- correct (all K2 / multi-GPU tests), 1.08 ms instead of 1.04 at N = 50 000, 0.43 instead of 0.36 at N = 30 000: the scan, the
// queue traffic and four more barriers per batch cost what the idle lanes had cost.
// And: the column BINNED by partition in global memory first (a kernel of its own: per-wave counts by ballot, then (value, sketch) runs at
// per-wave cursors; 12 bytes per value), then ranked bin by bin from the dense lists with 16384-slot tables -- correct, but the binning
// kernel alone took 0.54 ms at N = 50 000 (0.23 at 30 000) and the bin-ranking kernel 0.62 (0.36): 1.16 ms against 1.04.  The walking
// kernel stays; what it costs is ~84 dependent round trips per workgroup (three per batch of eight values and pass) with one 128 KiB-table
// workgroup per CU to hide them.)
constexpr uint32_t BS_SPLIT_SHIFT = 28, BS_RANK_MASK = (1u << BS_SPLIT_SHIFT) - 1u;
// ---- where the pieces of an announced output's fill lie (the riders below, the side fill, the FAST rank kernel): ONE definition.  The output pointer is
// only 4-byte aligned in general: `head` words (0 .. 3) in front of the 16-byte aligned body of `nb` vectors, at most three tail words behind it.  Piece p
// is the vectors [2048 p, 2048 (p + 1)) of the body; whoever writes piece 0 writes the head and tail words too (sp_fill_ends).
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
// s_waitcnt immediate of the gfx9 family (gfx950 among it): vmcnt = bits 3:0 and 15:14, expcnt = 6:4, lgkmcnt = 11:8 -- "every vector memory operation
// has returned", the other two counters not waited for (their maxima)
constexpr int BS_WAIT_VM0 = (0x7 << 4) | (0xF << 8);
#if defined(__HIP_DEVICE_COMPILE__) && !defined(__GFX9__)
#error "BS_WAIT_VM0 is the s_waitcnt encoding of the gfx9 family"
#endif
struct SpFillAddr { u32x4 *body; size_t nb; uint32_t head, v; };
constexpr size_t SP_PIECE_VECS = (size_t)SP_FILL_THREADS * SP_FILL_PER_THREAD;
__device__ __forceinline__ SpFillAddr sp_fill_addr(const SpRider &r) {
    const size_t head = min(r.cnt, (size_t)((16 - ((uintptr_t)r.out & 15)) & 15) / 4);
    return SpFillAddr{reinterpret_cast<u32x4 *>(r.out + head), (r.cnt - head) / 4, (uint32_t)head, r.vsrc ? r.vsrc[0] : r.vimm};
}
// non-temporal stores (as in sp_fill_kernel): 200 MB of output nobody reads again must not push the prepare's working set out of the MALL
__device__ __forceinline__ void sp_fill_store(const SpFillAddr &a, size_t i) { __builtin_nontemporal_store(u32x4{a.v, a.v, a.v, a.v}, &a.body[i]); }
__device__ __forceinline__ void sp_fill_ends(const SpRider &r, const SpFillAddr &a) {
    if (threadIdx.x < a.head) r.out[threadIdx.x] = a.v;
    const size_t tail0 = a.head + a.nb * 4;
    if (tail0 + threadIdx.x < r.cnt) r.out[tail0 + threadIdx.x] = a.v;
}

#ifdef D2G_RANK_TRACE
// variant builds only (tools/build_variant.sh ranktrace -DD2G_RANK_TRACE; tools/rank_trace.py): per-workgroup time stamps of the rank kernel --
// FAST: 0 start, 1 values loaded + table cleared, 2 claims done, 3 confirms done, 4 compaction done, 5 ids stored;
// general: 0 start, then per partition pass p (first four): 1+2p walk (load, claim, confirm, pending ids) done, 2+2p compaction + final ids done
__device__ unsigned long long g_rank_trace[8192 * 16];
#define RK_STAMP(k) do { if (threadIdx.x == 0 && blockIdx.x < 8192 && (k) < 16) g_rank_trace[blockIdx.x * 16 + (k)] = __builtin_amdgcn_s_memrealtime(); } while (0)
#else
#define RK_STAMP(k) do { } while (0)
#endif
template <bool MULTI, bool FAST, typename IdT = uint32_t>
__global__ __launch_bounds__(BS_RANK_THREADS) void bs_rank_kernel(const uint64_t *__restrict__ cols, size_t N, size_t Npad,
                                                                  uint32_t T, int logT, void *ids_void, uint32_t *colcnt,
                                                                  uint32_t *status, int tagbits_max, uint32_t S, int nsplit,
                                                                  uint32_t *__restrict__ owner_all, size_t ostride, SpRider fill, uint32_t fill_n) {
    extern __shared__ __attribute__((aligned(16))) uint32_t own[];        // Tl owner slots
    const uint32_t split = MULTI ? blockIdx.x / S : 0u;
    const size_t t = MULTI ? blockIdx.x - split * S : blockIdx.x;
    const uint32_t htag = (MULTI && nsplit > 1) ? split << BS_SPLIT_SHIFT : 0u;
    const uint64_t *col = cols + t * Npad;
    static_assert(!MULTI || sizeof(IdT) == 4, "bs_rank_kernel: the pending words and split tags of the MULTI kernel need 32-bit ids");
    IdT *ids = static_cast<IdT *>(ids_void) + t * Npad;
    const int tid = threadIdx.x;
    const int logTl = logT < BS_LOG_TLDS_MAX ? logT : BS_LOG_TLDS_MAX;
    const uint32_t Tl = 1u << logTl, mask = Tl - 1, nparts = MULTI ? (T >> logTl) : 1u;
    const uint32_t part_lo = MULTI ? split * (nparts / (uint32_t)nsplit) : 0u, part_hi = MULTI ? part_lo + nparts / (uint32_t)nsplit : 1u;
    __shared__ uint32_t wave_tot[BS_RANK_THREADS / 64];
    __shared__ uint32_t running;
    constexpr uint32_t BS_MAXFIX = 64;
    __shared__ uint32_t nfix, fix_j[BS_MAXFIX], fix_h[BS_MAXFIX];
    RK_STAMP(0);
    if (tid == 0) { running = 1; nfix = 0; }                             // id 0 is reserved for singletons
    const int lane = tid & 63, wave = tid >> 6;
    // owner_all (single-partition kernels of sets that take the sparse path): owner[t][r - 1] = the sketch that owns the slot of the value
    // ranked r -- ONE holder of every shared value, for free: the sparse path's link passes (sp_olink_kernel) compare every holder with its
    // value's owner instead of grouping the holders in LDS again
    uint32_t *owner = (owner_all && nsplit == 1) ? owner_all + t * ostride : nullptr;      // (one workgroup per column: `running` numbers the column's shared values 1 .. D2)
    const int ib0 = 32 - __clz((uint32_t)N);
    const uint32_t ownmask = (ib0 >= 32 ? 0xFFFFFFFFu : (1u << ib0) - 1u) & ~BS_DUP;

    // the compaction of one table pass: slots whose value occurs >= 2 times get the next dense ranks,
    // singletons BS_UNIQ
    auto compact = [&]() {
        // one block-wide prefix over per-thread counts (a thread owns slots tid, tid + 1024, ...): three
        // barriers per pass instead of three per 1024 slots; any bijection onto 1..#dups is a valid ranking
        uint32_t cnt = 0;
        for (uint32_t h = tid; h < Tl; h += BS_RANK_THREADS) {
            const uint32_t cur = own[h];
            cnt += (cur != BS_EMPTY) && (cur & BS_DUP);
        }
        uint32_t incl = cnt;
        for (int o = 1; o < 64; o <<= 1) { const uint32_t x = __shfl_up(incl, o); if (lane >= o) incl += x; }
        if (lane == 63) wave_tot[wave] = incl;
        __syncthreads();
        uint32_t woff = 0, tot = 0;
        for (int w = 0; w < BS_RANK_THREADS / 64; ++w) {
            const uint32_t x = wave_tot[w];
            if (w < wave) woff += x;
            tot += x;
        }
        uint32_t r = running + woff + (incl - cnt);
        for (uint32_t h = tid; h < Tl; h += BS_RANK_THREADS) {
            const uint32_t cur = own[h];
            if (cur != BS_EMPTY) {
                if ((cur & BS_DUP) && owner) owner[r - 1] = cur & ownmask;
                own[h] = (cur & BS_DUP) ? (r++ | htag) : BsId<IdT>::UNIQ;
            }
        }
        __syncthreads();
        if (tid == 0) running += tot;
        __syncthreads();
    };
    // Owner slot = [DUP:1][tag][owner sketch index:ib].  The tag (hash bits below the slot bits) lets a probe step
    // over a slot that holds a DIFFERENT value without fetching the owner's value from the column: only a
    // tag match -- practically always a true repeat -- pays the global load that decides equality exactly.
    // The all-ones index is never a sketch index (2^ib > N), so EMPTY cannot be mistaken for an owner.
    const int ib = 32 - __clz((uint32_t)N);
    const uint32_t idxmask = (ib >= 32 ? 0xFFFFFFFFu : (1u << ib) - 1u) & ~BS_DUP;
    // tagbits_max < 31 only in tests (D2G_BS_TAGBITS): a narrow tag makes tag collisions common
    const uint32_t tagfield = ~BS_DUP & ~idxmask & (ib + tagbits_max >= 31 ? 0xFFFFFFFFu : (1u << (ib + tagbits_max)) - 1u);
    auto slot_word = [&](uint64_t prod, uint32_t j) {                     // prod = v * K (bs_hash's product)
        return j | ((uint32_t)((prod << logT) >> 33) & tagfield);         // the 31 bits below the slot bits, cut to the field
    };
    // at most Tl probes: a partition that receives more than Tl distinct values (a skewed / adversarial
    // column; T >= 1.5 N only bounds the AVERAGE load) must not spin forever.  The overflow is
    // reported through *status; the host then falls back to the DIRECT algorithm or fails loudly.
    auto insert = [&](uint64_t v, uint32_t j, uint32_t h) {
        const uint32_t mine = slot_word(v * 0x9E3779B97F4A7C15ull, j);
        for (uint32_t probes = 0; probes < Tl; ++probes) {
            const uint32_t cur = atomicCAS(&own[h], BS_EMPTY, mine);
            if (cur == BS_EMPTY) return h;                                // first occurrence: we own the slot
            if (!((cur ^ mine) & tagfield) && col[cur & idxmask] == v) {  // same value seen again
                if (!(cur & BS_DUP)) atomicOr(&own[h], BS_DUP);
                return h;
            }
            h = (h + 1) & mask;
        }
        atomicOr(status, 1u);
        return h;                                                         // garbage id, flagged
    };

    constexpr int PF = BS_RANK_PF;      // values a thread keeps in registers (fast path: N <= 12288, one partition)
    if constexpr (FAST) {
        // every value is fetched BEFORE the probe chains (a load inside the chain exposed a full HBM/L2 round
        // trip per value) and its slot stays in a register until the ids are written.
        // Two phases.  (1) claim: probe with LDS compare-and-swaps only; stop at the first slot that is won or
        // whose tag matches (the CANDIDATE: same value, up to a tag collision).  (2) confirm: the owners' values
        // of the candidates are fetched a few at a time -- independent loads, one exposed round trip per batch
        // instead of one per value -- and compared exactly; a confirmed repeat flags the slot, the rare tag
        // collision resumes the exact serial chain behind it.  Every thread holding the same value stops at the
        // same candidate (claimed slots never change owner or tag), so the outcome is the exact ranking.
        // (Probing a thread's values TOGETHER, round by round, was measured too: it needs > 64 VGPRs, i.e. one
        // workgroup per CU instead of two, and is slower -- profiles/r02_k2_experiments.txt.)
        //
        // The announced fill's first fill_n pieces (SpAnnounced::take_first), in equal runs of `per` <= SP_RANK_FILL_PER_WG pieces per workgroup: one
        // 16-byte non-temporal store per thread in front of each probe chain of the claim loop.  THERE and nowhere later: loads and stores share the one
        // VM counter, so the confirm phase's wait for its owner fetches also waits for every store issued before them -- in the claim phase, LDS round
        // trips only, nothing waits for them by name (not free either: the trace in profiles/k2_rank_fill.txt section 6).  Set up HERE, in front of the value loads: the fill value is one scalar load, and
        // workgroup 0's head and tail words are on their way with the values.  fa.body = this workgroup's run, fcnt its vectors (nothing rides: 0)
        SpFillAddr fa{nullptr, 0, 0u, 0u};
        uint32_t fcnt = 0;
        if (fill_n) {
            fa = sp_fill_addr(fill);
            if (blockIdx.x == 0) sp_fill_ends(fill, fa);
            const uint32_t per = (fill_n + gridDim.x - 1) / gridDim.x;
            const size_t p0 = (size_t)blockIdx.x * per;
            const size_t b0 = min(p0 * SP_PIECE_VECS, fa.nb), b1 = min(min(p0 + per, (size_t)fill_n) * SP_PIECE_VECS, fa.nb);
            fa.body += b0;
            fcnt = b1 > b0 ? (uint32_t)(b1 - b0) : 0u;                    // (<= SP_RANK_FILL_PER_WG pieces = PF x 1024 vectors: the host's bound)
        }
        uint64_t v[PF];
        uint32_t hs[PF];
#pragma unroll
        for (int i = 0; i < PF; ++i) {
            const size_t j = (size_t)i * BS_RANK_THREADS + tid;
            v[i] = j < N ? col[j] : 0;
        }
        for (uint32_t h = tid; h < Tl; h += BS_RANK_THREADS) own[h] = BS_EMPTY;
        __syncthreads();
        // every value has arrived (they were requested together, in front of the table clear) before the first probe chain -- said HERE, outside any branch:
        // the claim loop below issues the fill's stores between its chains, and a wait for value i placed by the compiler behind store i - 1 (stores and
        // loads share the one VM counter, and it cannot count across the loop's branches) would be a wait for that store's whole round trip to the HBM
        // (Unconditional: under `if (fill_n)` the compiler no longer knows at the join that the loads are in, and puts the waits back behind every store.)
        __builtin_amdgcn_s_waitcnt(BS_WAIT_VM0);
        RK_STAMP(1);
        uint32_t candidate = 0;                                           // bit i: value i stopped at a tag match
        // (round 6: per-workgroup time stamps -- tools/rank_trace.py, profiles/r06_rank_trace.txt -- put this claim phase at 10.7 of the workgroup's 21 us at
        // config 3 (6.1 of 15.7 on unrelated sketches): a quarter of the LDS atomic rate, i.e. the dependent compare-and-swap round trips of waves whose
        // every step waits for its slowest lane.  Two chains per thread in flight, interleaved, were measured: 13.2 us)
#pragma unroll
        for (int i = 0; i < PF; ++i) {
            const size_t j = (size_t)i * BS_RANK_THREADS + tid;
            hs[i] = 0;
            if ((uint32_t)(i * BS_RANK_THREADS + tid) < fcnt) sp_fill_store(fa, (uint32_t)(i * BS_RANK_THREADS + tid));
            if (j < N) {
                const uint64_t prod = v[i] * 0x9E3779B97F4A7C15ull;
                const uint32_t mine = slot_word(prod, (uint32_t)j);
                uint32_t h = (uint32_t)(prod >> (64 - logT)) & mask, probes = 0;
                for (; probes < Tl; ++probes) {
                    const uint32_t cur = atomicCAS(&own[h], BS_EMPTY, mine);
                    if (cur == BS_EMPTY) break;
                    if (!((cur ^ mine) & tagfield)) { candidate |= 1u << i; break; }
                    h = (h + 1) & mask;
                }
                if (probes == Tl) atomicOr(status, 1u);
                hs[i] = h;
            }
        }
        // (CB = 3 / 4 / 6 under amdgpu_waves_per_eu(8) with the slots packed two per register -- 64 VGPRs, 4-6 spilled -- measured in round 5:
        // 53.1 -> 56.3 us for CB = 4, step 0.290 -> 0.294 ms.  Without a single candidate (a matrix of unrelated sketches) the kernel takes 38 us:
        // the confirm phase costs 15 us for ten million candidates whatever its batch size)
        constexpr int CB = 2;                                             // owner fetches in flight per thread
        uint32_t redo = 0;
#ifdef D2G_RANK_TRACE
        __syncthreads();
        RK_STAMP(2);
#endif
#pragma unroll
        for (int c = 0; c < PF; c += CB) {
            uint32_t o[CB];
            uint64_t w[CB];
#pragma unroll
            for (int g = 0; g < CB; ++g)
                if (candidate >> (c + g) & 1) o[g] = own[hs[c + g]];
#pragma unroll
            for (int g = 0; g < CB; ++g)
                if (candidate >> (c + g) & 1) w[g] = col[o[g] & idxmask];
#pragma unroll
            for (int g = 0; g < CB; ++g)
                if (candidate >> (c + g) & 1) {
                    if (w[g] == v[c + g]) {
                        if (!(o[g] & BS_DUP)) atomicOr(&own[hs[c + g]], BS_DUP);
                    } else redo |= 1u << (c + g);
                }
            __builtin_amdgcn_sched_barrier(0);                            // one batch of fetches at a time (VGPRs: 2 workgroups per CU)
        }
        // tag collisions (about one value in 10^5): the exact serial chain from the value's home slot; it walks past
        // the false candidate.  Their slots go through a small LDS list instead of hs[] (conditional updates of the
        // register array made the compiler keep several copies of it).
        const uint32_t skip = redo;
        while (redo) {
            const int i = __ffs(redo) - 1;
            redo &= redo - 1;
            const uint32_t j = (uint32_t)i * BS_RANK_THREADS + tid;
            const uint64_t vv = col[j];
            const uint32_t h2 = insert(vv, j, bs_hash(vv, logT) & mask);
            const uint32_t k = atomicAdd(&nfix, 1u);
            if (k < BS_MAXFIX) { fix_j[k] = j; fix_h[k] = h2; }
            else atomicOr(status, 1u);                                    // cannot happen by chance; the host falls back to DIRECT
        }
        __syncthreads();
        RK_STAMP(3);
        compact();
        RK_STAMP(4);
#pragma unroll
        for (int i = 0; i < PF; ++i) {
            const size_t j = (size_t)i * BS_RANK_THREADS + tid;
            if (j < N && !(skip >> i & 1)) ids[j] = (IdT)own[hs[i]];      // (16-bit ids: a wave still writes 64 consecutive words -- lane = sketch, packing two would cost a cross-lane move per value)
        }
#ifdef D2G_RANK_TRACE
        __syncthreads();
        RK_STAMP(5);
#endif
        for (uint32_t k = tid; k < nfix && k < BS_MAXFIX; k += BS_RANK_THREADS) ids[fix_j[k]] = (IdT)own[fix_h[k]];
        if (tid == 0) { colcnt[t * BS_CC_STRIDE] = running - 1; colcnt[t * BS_CC_STRIDE + 5] = running - 1; }   // #values shared by >= 2 sketches ([5]: a copy the column plan leaves alone -- sp_sample_fin_kernel reads it beside that kernel)
        return;
    }

    // split workgroups write the same ids[] concurrently: a pending word names its partition (bits 15..29; N < 2^28 there), so
    // that a pass only resolves its own, and nobody initialises ids[] for the others (the buffer is zeroed once, at
    // allocation; afterwards it only ever holds final ids, which have bit 30 clear)
    const bool tagged = MULTI && nsplit > 1;
    for (uint32_t part = part_lo; part < part_hi; ++part) {
        const uint32_t ptag = BS_PENDING | (tagged ? part << 15 : 0u);
        for (uint32_t h = tid; h < Tl; h += BS_RANK_THREADS) own[h] = BS_EMPTY;
        __syncthreads();
        // values are fetched PG at a time before their probe chains, and a batch goes through the same two phases as the
        // fast path: claim with LDS compare-and-swaps only, then confirm the candidates with their owner fetches in flight
        // together (with one 128 KiB-table workgroup per CU nothing else hides a round trip)
        constexpr int PG = 8;
        // which of this thread's values the pass placed, a byte per batch (up to eight batches: 65 536 sketches): the pass's second loop then
        // fetches only THEIR pending words instead of every id of the column (round 6: 1033 -> 992 us at 50 000 sketches).
        // (Round 6 also measured HASHED later passes -- the first pass leaves the top 30 bits of every later value's hash product in ids[], the later
        // passes walk those 4-byte words instead of the 8-byte values, only tag matches fetch their value: correct, and SLOWER -- first pass 47 -> 74 us,
        // later ones 43 -> 48: the walk is not bound by the bytes it reads but by its claim / confirm round trips; profiles/r06_rank_trace.txt)
        const bool mine_known = N <= (size_t)8 * PG * BS_RANK_THREADS;
        unsigned long long mine_all = 0;
        int batch = 0;
        for (size_t j0 = 0; j0 < N; j0 += (size_t)PG * BS_RANK_THREADS) {
            uint64_t v[PG];
            uint32_t hs[PG];
#pragma unroll
            for (int i = 0; i < PG; ++i) {
                const size_t j = j0 + (size_t)i * BS_RANK_THREADS + tid;
                v[i] = j < N ? col[j] : 0;
            }
            uint32_t mineb = 0, candidate = 0, redo = 0;
#pragma unroll
            for (int i = 0; i < PG; ++i) {
                const size_t j = j0 + (size_t)i * BS_RANK_THREADS + tid;
                const uint64_t prod = v[i] * 0x9E3779B97F4A7C15ull;
                const uint32_t hh = (uint32_t)(prod >> (64 - logT));
                hs[i] = 0;
                if (j < N && (!MULTI || (hh >> logTl) == part)) {
                    mineb |= 1u << i;
                    const uint32_t mine = slot_word(prod, (uint32_t)j);
                    uint32_t h = hh & mask, probes = 0;
                    for (; probes < Tl; ++probes) {
                        const uint32_t cur = atomicCAS(&own[h], BS_EMPTY, mine);
                        if (cur == BS_EMPTY) break;
                        if (!((cur ^ mine) & tagfield)) { candidate |= 1u << i; break; }
                        h = (h + 1) & mask;
                    }
                    if (probes == Tl) atomicOr(status, 1u);
                    hs[i] = h;
                }
            }
            {
                uint32_t o[PG];
                uint64_t w[PG];
#pragma unroll
                for (int i = 0; i < PG; ++i)
                    if (candidate >> i & 1) o[i] = own[hs[i]];
#pragma unroll
                for (int i = 0; i < PG; ++i)
                    if (candidate >> i & 1) w[i] = col[o[i] & idxmask];
#pragma unroll
                for (int i = 0; i < PG; ++i)
                    if (candidate >> i & 1) {
                        if (w[i] == v[i]) { if (!(o[i] & BS_DUP)) atomicOr(&own[hs[i]], BS_DUP); }
                        else redo |= 1u << i;
                    }
            }
            // MULTI: a slot written in this pass carries BS_PENDING (never set in a final id: ranks stay below 2^30, BS_UNIQ is
            // bit 31), so that the pass's second loop finds its values in ids[] alone, without re-reading and re-hashing the
            // column -- the kernel is bound by its column reads at this size.  Pass 0 writes every id (0 = not yet placed).
#pragma unroll
            for (int i = 0; i < PG; ++i) {
                const size_t j = j0 + (size_t)i * BS_RANK_THREADS + tid;
                if ((mineb & ~redo) >> i & 1) ids[j] = (IdT)(hs[i] | (MULTI ? ptag : 0u));
                else if (MULTI && !tagged && part == 0 && j < N && !(redo >> i & 1)) ids[j] = 0;
            }
            while (redo) {                                                // tag collisions: the exact chain from the home slot
                const int i = __ffs(redo) - 1;
                redo &= redo - 1;
                const size_t j = j0 + (size_t)i * BS_RANK_THREADS + tid;
                const uint64_t vv = col[j];
                ids[j] = (IdT)(insert(vv, (uint32_t)j, bs_hash(vv, logT) & mask) | (MULTI ? ptag : 0u));
            }
            if (batch < 8) mine_all |= (unsigned long long)mineb << (8 * batch);
            ++batch;
        }
        __syncthreads();
        RK_STAMP(1 + 2 * (part - part_lo));
        compact();
        batch = 0;
        for (size_t j0 = 0; j0 < N; j0 += (size_t)PG * BS_RANK_THREADS, ++batch) {
            uint32_t sl[PG];
            const uint32_t mb = mine_known ? (uint32_t)(mine_all >> (8 * batch)) & 0xFFu : 0xFFu;
#pragma unroll
            for (int i = 0; i < PG; ++i) {
                const size_t j = j0 + (size_t)i * BS_RANK_THREADS + tid;
                sl[i] = (j < N && (mb >> i & 1)) ? ids[j] : 0;
            }
#pragma unroll
            for (int i = 0; i < PG; ++i) {
                const size_t j = j0 + (size_t)i * BS_RANK_THREADS + tid;
                if (j < N && (mb >> i & 1) && (mine_known || !MULTI || (tagged ? (sl[i] & ~0x7FFFu) == ptag : (sl[i] & BS_PENDING) != 0)))
                    ids[j] = (IdT)own[sl[i] & (tagged ? 0x7FFFu : ~BS_PENDING)];
            }
        }
        __syncthreads();
        RK_STAMP(2 + 2 * (part - part_lo));
    }
    if (tid == 0) { colcnt[t * BS_CC_STRIDE + split] = running - 1; if (nsplit == 1) colcnt[t * BS_CC_STRIDE + 5] = running - 1; }   // #values shared by >= 2 sketches (this split's)
}

// ------------------------------------------------------------------ 2. 32 x nbits bit transpose
// thread (tb, j): reads the ids of sketch j for 32 consecutive registers, writes nbits words.
__device__ __forceinline__ int live_planes(const uint32_t *meta, int tb) {
    const uint32_t md = meta[tb];                      // max over the group's columns of (#shared values D2) + 1
    return md <= 1 ? 1 : 32 - __clz(md);              // smallest nb with 2^nb >= D2 + 2: ranks 1..D2, 0 and 2^nb-1 all distinct
}

// first slot of group tb in the compact plane stream = sum of the live plane counts of the groups before it
__device__ __forceinline__ size_t stream_slot(const uint32_t *meta, int tb) {
    size_t q = 0;
    for (int t = 0; t < tb; ++t) q += (size_t)live_planes(meta, t);     // uniform scalar loop, ntb = S/32 is small
    return q;
}

// the same sum with ONE round trip: lane t of the calling wave takes group t, the wave adds up (the scalar loop above waits out one
// scalar load per group: up to 31 dependent round trips in front of a kernel's first store).  Every lane of the wave must be here.
__device__ __forceinline__ size_t stream_slot_wave(const uint32_t *meta, int tb) {
    const int lane = threadIdx.x & 63;
    uint32_t q = 0;
    for (int t0 = 0; t0 < tb; t0 += 64) {
        const int t = t0 + lane;
        uint32_t v = t < tb ? (uint32_t)live_planes(meta, t) : 0u;
        for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
        q += v;
    }
    return (size_t)__builtin_amdgcn_readfirstlane(q);
}

// ------------------------------------------------------------------ riders
// The fill of an upper-triangle launch (every output = "no register equal", 4 bytes per pair: 200 MB at config 3, 31 us of pure HBM
// writes) depends on nothing the prepare computes, and six kernels of the prepare chain are one to forty workgroups waiting out
// dependent round trips on an otherwise idle chip (column plan, flatten, count, attach, scan, place: 36 us together at config 3; in the merged schedule
// the first two hosts are the launches that CONTAIN the column plan and flatten: sp_link0_plan_kernel, bs_planes_flatten_kernel -- in schedule 2, where the
// planes stand behind emit's workgroups, the second is sp_flatten_kernel itself again).  When the
// output is announced ahead of the prepare (d2g_cmp_ut_announce_dev) those kernels are launched with extra workgroups BEHIND their own --
// the dispatcher starts workgroups in index order, the kernel's own work is never queued behind a rider -- each writing one 32 KB piece.
// (The same fill on a second stream was measured in rounds 4 and 5: the two cross-stream dependencies cost more than the fill.)
// In front of the riders stands the FAST rank kernel (bit 64 of D2G_SP_RIDE, D2G_SP_RANK_SHARE): no rider workgroup fits beside it, every wave slot is
// taken, but its own threads write the FIRST pieces [0, n) from inside their claim loop (bs_rank_kernel; n <= six pieces per column: all of config 3's
// 6 104), and the riders here carry what is left, by their weights, from piece n on.  Where a piece lies is defined once, in sp_fill_addr / sp_fill_ends
// above the rank kernel; SpFilled::pieces stays the prefix the launch skips (what it gives and takes: profiles/k2_rank_fill.txt).
__device__ __forceinline__ void sp_ride_piece(const SpRider &r, size_t piece) {
    const SpFillAddr a = sp_fill_addr(r);
    const size_t end = min((piece + 1) * SP_PIECE_VECS, a.nb);
    for (size_t i = piece * SP_PIECE_VECS + threadIdx.x; i < end; i += blockDim.x) sp_fill_store(a, i);
    if (piece == 0) sp_fill_ends(r, a);
}
__device__ __forceinline__ void sp_ride(const SpRider &r) { sp_ride_piece(r, (size_t)r.piece0 + (blockIdx.x - r.own)); }
#define SP_RIDE_OR_WORK(r) do { if (blockIdx.x >= (r).own) { sp_ride(r); return; } } while (0)
// A LARGE announced output (>= SP_SIDE_FILL_PIECES pieces: 1 GB, ~23 000 sketches) is filled by a kernel of its own on a second stream, beside the
// rank kernel: that one waits on its LDS tables for 1.0 ms at 50 000 sketches with the HBM almost idle, while the 5 GB fill spread over the six
// hosts made each of them last 110-180 us (0.75 ms together).  Two cross-stream dependencies (~10 us) that a 200 MB fill does not earn back
// (measured in rounds 4 and 5) and a 5 GB one does many times over.
__global__ __launch_bounds__(256) void sp_side_fill_kernel(SpRider r, uint32_t pieces) {
    for (size_t p = blockIdx.x; p < pieces; p += gridDim.x) sp_ride_piece(r, p);
}
constexpr uint32_t SP_SIDE_FILL_PIECES = 32768;
// How hard the side fill may pull: unthrottled (one workgroup per 32 KB piece, 5.5 TB/s) it stretched the rank kernel beside it from 1.04 to 1.63 ms at
// 50 000 sketches (step 2.54 ms); with persistent workgroups looping over the pieces -- 64 / 128 / 192 / 256 / 384 of them: 2.4 / 3.7 / 4.4 / 4.5 / 5.1 TB/s --
// the two end together at 128 (rank 1.39, fill 1.36 ms: step 2.27 ms).  So: the fewest workgroups whose rate still finishes the fill within 1.3 x the rank
// kernel's own time (21 ns per sketch at S = 1024, measured at 50 000), everything the chip has when even that is too slow (100 000 sketches on).
inline unsigned sp_side_fill_grid(const d2g_ctx *ctx, uint32_t pieces, size_t words, size_t N, size_t S) {
    const double need = (double)words * 4.0 / (1.3 * 21.0 * (double)N * ((double)S / 1024.0));     // bytes per ns = GB/s
    const unsigned cus = (unsigned)ctx->num_cus;
    const unsigned g = need <= 3700.0 ? cus / 2 : need <= 4400.0 ? cus * 3 / 4 : need <= 5000.0 ? cus * 3 / 2 : pieces;
    return std::max(1u, std::min<unsigned>(pieces, g));
}

// ------------------------------------------------------------------ 1b. column plan
// One workgroup: a kernel of its own in the classic schedule, block 0 of the link launch in the merged one (sp_link0_plan_kernel, d2g_k2_sparse.h: it
// needs nothing but the rank kernel's counts, and nothing in that launch needs what it writes).  (Letting the LAST workgroup of the rank kernel do this -- ticket counter -- was
// measured: with an agent-scope fence per workgroup the rank kernel went 52 -> 111 us at config 3, every fence writes the
// XCD's L2 back; fence-free, with returning device-scope atomics for the counts and the ticket, 52 -> 81 us.  The
// separate launch costs ~7 us.)  Input: colcnt[t][h] = shared values split h of the rank kernel found in column t.  Output:
//   colcnt[t][0..nsplit)  exclusive prefix over the splits (the rank offset bs_planes_kernel adds), colcnt[t][4] = D2(t)
//   perm[slot]            the column that sits in register slot `slot` of the operand (~0 = padding): the columns in
//                         DESCENDING order of their live-plane class (stable), so that a 32-register group holds
//                         columns of similar plane counts and meta[tb] -- a maximum -- does not let one busy column tax
//                         31 quiet ones.  Equality counts are sums over columns (reference src/cmp_core.cpp:461,506):
//                         any permutation gives the same counts.
//   meta[tb]              max over the group's columns of D2 + 1 (also to the export target, with the status word)
constexpr int BS_PLAN_THREADS = 1024;
constexpr int BS_PLAN_MAXS = 4096;                // slots sorted in LDS; larger sketches keep the identity order
constexpr uint32_t BS_NOCOL = 0xFFFFFFFFu;
__device__ __forceinline__ int plane_class(uint32_t d2) { return d2 == 0 ? 1 : 32 - __clz(d2 + 1); }   // = live_planes(D2 + 1)

// The plan's body for a block of T threads (T = BS_PLAN_THREADS in the kernel of its own; 256 as block 0 of the merged link launch, sp_link0_plan_kernel):
// correct for any Spad <= BS_PLAN_MAXS, and for the identity order beyond.  LDS (the caller's): d2s[Spad], perm_s[Spad], cell[32 * ceil(Spad / 64)],
// wave_tot[T / 64] -- bs_plan_lds_words(Spad) words in all, laid out by BsPlanLds.
struct BsPlanArgs {
    uint32_t *colcnt; uint32_t S; int ntb, nsplit; uint32_t *perm, *meta; const uint32_t *status; uint32_t *ex_meta, *ex_status; int sort;
};
struct BsPlanLds { uint32_t *d2s, *cell, *wave_tot; uint16_t *perm_s; };
__host__ __device__ inline uint32_t bs_plan_sorted(uint32_t Spad, int sort) { return sort && Spad <= (uint32_t)BS_PLAN_MAXS; }
__host__ __device__ inline size_t bs_plan_lds_words(uint32_t Spad, int sort) {      // (identity order: no LDS)
    return bs_plan_sorted(Spad, sort) ? (size_t)Spad + 32 * (size_t)((Spad + 63) / 64) + 16 + (Spad + 1) / 2 : 0;
}
__device__ __forceinline__ BsPlanLds bs_plan_lds(uint32_t *base, uint32_t Spad) {
    const uint32_t ncell = 32 * ((Spad + 63) / 64);
    return BsPlanLds{base, base + Spad, base + Spad + ncell, reinterpret_cast<uint16_t *>(base + Spad + ncell + 16)};
}
template <int T>
__device__ __forceinline__ void bs_colplan_body(const BsPlanArgs &pa, const BsPlanLds &l) {
    static_assert(T % 64 == 0 && T <= 1024 && BS_PLAN_MAXS % T == 0 && (32 * (BS_PLAN_MAXS / 64)) % T == 0, "bs_colplan_body: block size");
    uint32_t *const colcnt = pa.colcnt, *const perm = pa.perm, *const meta = pa.meta, *const ex_meta = pa.ex_meta;
    const uint32_t S = pa.S;
    const int ntb = pa.ntb, nsplit = pa.nsplit;
    uint32_t *const d2s = l.d2s, *const cell = l.cell, *const wave_tot = l.wave_tot;
    uint16_t *const perm_s = l.perm_s;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint32_t Spad = (uint32_t)ntb * 32u;
    auto column_total = [&](uint32_t t) {             // D2 of column t; leaves the per-split offsets behind
        uint32_t run = 0;
        for (int h = 0; h < nsplit; ++h) { const uint32_t c = colcnt[(size_t)t * BS_CC_STRIDE + h]; colcnt[(size_t)t * BS_CC_STRIDE + h] = run; run += c; }
        colcnt[(size_t)t * BS_CC_STRIDE + 4] = run;
        return run;
    };
    if (tid == 0 && pa.ex_status) *pa.ex_status = *pa.status;
    if (!bs_plan_sorted(Spad, pa.sort)) {              // identity order
        for (uint32_t t = tid; t < S; t += T) (void)column_total(t);
        for (uint32_t p = tid; p < Spad; p += T) perm[p] = p < S ? p : BS_NOCOL;
        __threadfence();
        __syncthreads();
        for (int g = tid; g < ntb; g += T) {
            uint32_t mx = 0;
            for (uint32_t x = 0; x < 32; ++x) { const uint32_t t = (uint32_t)g * 32 + x; if (t < S) mx = max(mx, colcnt[(size_t)t * BS_CC_STRIDE + 4]); }
            meta[g] = mx + 1;
            if (ex_meta) ex_meta[g] = mx + 1;
        }
        return;
    }
    const uint32_t nchunk = (Spad + 63) / 64, ncell = 32 * nchunk;
    for (uint32_t c = tid; c < ncell; c += T) cell[c] = 0;
    __syncthreads();
    constexpr int IT = BS_PLAN_MAXS / T;
    uint32_t mine[IT];                                                 // (cell << 6 | rank inside the cell: one register per slot -- the merged link launch shares its register budget with the link pass)
#pragma unroll
    for (int it = 0; it < IT; ++it) {
        const uint32_t t = (uint32_t)it * T + tid;                    // a wave covers the 64 consecutive slots of chunk t / 64
        mine[it] = 0;
        if (t - lane < Spad) {                                         // wave-uniform
            uint32_t d2 = 0;
            int cls = 0;                                               // class 0 = padding: sorted behind every real column
            if (t < S) { d2 = column_total(t); cls = plane_class(d2); }
            if (t < Spad) d2s[t] = d2;
            unsigned long long todo = __ballot(t < Spad);
            while (todo) {                                             // one round per distinct class in the wave
                const int k = __shfl(cls, __ffsll((long long)todo) - 1);
                const unsigned long long m = __ballot(cls == k && t < Spad);
                const uint32_t ci = (uint32_t)(31 - k) * nchunk + t / 64;   // descending class, ascending slot
                if (cls == k && t < Spad) mine[it] = ci << 6 | (uint32_t)__popcll(m & ((1ull << lane) - 1));
                if (lane == 0) cell[(uint32_t)(31 - k) * nchunk + (t - lane) / 64] = __popcll(m);
                todo &= ~m;
            }
        }
    }
    __syncthreads();
    {   // exclusive prefix over the cells (<= 2048): CPT consecutive ones per thread
        constexpr int CPT = 32 * (BS_PLAN_MAXS / 64) / T;
        const uint32_t c0 = (uint32_t)CPT * tid;
        uint32_t v[CPT], sum = 0;
#pragma unroll
        for (int x = 0; x < CPT; ++x) { v[x] = c0 + x < ncell ? cell[c0 + x] : 0u; sum += v[x]; }
        uint32_t incl = sum;
        for (int o = 1; o < 64; o <<= 1) { const uint32_t x = __shfl_up(incl, o); if (lane >= o) incl += x; }
        if (lane == 63) wave_tot[wave] = incl;
        __syncthreads();
        uint32_t ex = incl - sum;
        for (int w = 0; w < wave; ++w) ex += wave_tot[w];
#pragma unroll
        for (int x = 0; x < CPT; ++x) { if (c0 + x < ncell) cell[c0 + x] = ex; ex += v[x]; }
    }
    __syncthreads();
#pragma unroll
    for (int it = 0; it < IT; ++it) {
        const uint32_t t = (uint32_t)it * T + tid;
        if (t < Spad) perm_s[cell[mine[it] >> 6] + (mine[it] & 63u)] = (uint16_t)t;
    }
    __syncthreads();
    for (uint32_t p = tid; p < Spad; p += T) { const uint32_t t = perm_s[p]; perm[p] = t < S ? t : BS_NOCOL; }
    for (int g = tid; g < ntb; g += T) {
        uint32_t mx = 0;
        for (uint32_t x = 0; x < 32; ++x) mx = max(mx, d2s[perm_s[(uint32_t)g * 32 + x]]);
        meta[g] = mx + 1;
        if (ex_meta) ex_meta[g] = mx + 1;
    }
}

__global__ __launch_bounds__(BS_PLAN_THREADS) void bs_colplan_kernel(BsPlanArgs pa, SpRider rider) {
    SP_RIDE_OR_WORK(rider);
    extern __shared__ __attribute__((aligned(16))) uint32_t plan_lds[];
    bs_colplan_body<BS_PLAN_THREADS>(pa, bs_plan_lds(plan_lds, (uint32_t)pa.ntb * 32u));
}

// Writes both forms of the operand:
//   planes  [ntb][nbits_cap+1][Nstride]  fixed geometry (a function of N only): row-coded id planes + the unique plane in the
//                                        last slot -- the form ranks exchange (independent per group);
//   stream  [sum_tb nbits_tb][2][Nstride] what the pair kernel walks: only the LIVE planes, in group order, each as the
//                                        row-coded words followed by the column-coded words, so that the kernel's operand
//                                        pointer simply advances by one block per plane (no per-plane address selection).
// Register slot x of group tb holds column perm[32 tb + x] (bs_colplan_kernel).
constexpr int BS_FORM_STREAM = 1, BS_FORM_EXCHANGE = 2;
constexpr size_t BS_SLACK = 64;          // words behind position Npad of every plane (Nstride = Npad + BS_SLACK)
struct BsPlanesArgs {
    const void *ids; size_t N, Npad; uint32_t *planes, *stream; size_t Nstride; int nbits_cap; const uint32_t *meta; int forms;
    const uint32_t *perm, *colcnt, *sperm;
};
BsPlanesArgs planes_args_of(const d2g_cmp_set *set, uint32_t *planes, int forms) {
    return BsPlanesArgs{set->d_ids.get(), set->N, set->Npad, planes, set->d_stream, set->Nstride, set->nbits_cap, set->d_meta, forms, set->d_perm, set->d_colcnt, nullptr};
}
// the body of workgroup (bx, tb) of the grid ceil(Nstride / 256) x ntb: 256 threads (bs_planes_kernel; the merged planes launch, bs_planes_flatten_kernel;
// `tid`: the thread's index among them where the block is larger -- sp_emit_kernel<IdT, true> runs two of these bodies in one block of 512, whole waves each)
// (16-bit ids: one 2-byte load per lane and column, a wave reads 128 consecutive bytes.  Measured and dropped: TWO adjacent positions per thread -- one 32-bit
// load holds both ids, the bit transpose runs on the packed words (bit b and bit b + 16), the two words of a plane leave as one 8-byte store; half the
// workgroups and half the load instructions -- the planes launch of the merged schedule took 19.6 us instead of 17.5 at config 3 (32-bit ids: 18.4):
// the same VALU work in half as many waves hides the loads worse.  profiles/k2_id16.txt)
template <bool SPLIT, typename IdT = uint32_t>
__device__ __forceinline__ void bs_planes_body(const BsPlanesArgs &a, size_t bx, size_t tb, uint32_t tid = threadIdx.x) {
    static_assert(!SPLIT || sizeof(IdT) == 4, "bs_planes_body: split ranks are 32-bit ids");
    constexpr int UBIT = BsId<IdT>::UBIT;
    const IdT *__restrict__ ids = static_cast<const IdT *>(a.ids);
    const uint32_t *__restrict__ meta = a.meta, *__restrict__ perm = a.perm, *__restrict__ colcnt = a.colcnt, *__restrict__ sperm = a.sperm;
    uint32_t *__restrict__ planes = a.planes, *__restrict__ stream = a.stream;
    const size_t N = a.N, Npad = a.Npad, Nstride = a.Nstride;
    const int nbits_cap = a.nbits_cap, forms = a.forms;
    const size_t jpos = bx * 256 + tid;           // position in the operand
    const size_t slot = (forms & BS_FORM_STREAM) ? stream_slot_wave(meta, (int)tb) : 0;     // (every lane still here)
    if (jpos >= Nstride) return;
    // sperm: the operand written in another order -- position p holds sketch sperm[p] (stream form only; unused: the sparse path permutes the finished stream)
    const size_t j = sperm ? (size_t)sperm[jpos] : jpos;          // 0xFFFFFFFF (padding) fails j < N below
    const int nbits = live_planes(meta, (int)tb);
    // the group's 32 columns: two s_load_dwordx16 (constant address space: never written while this kernel runs), all in
    // flight before the first id is requested
    typedef const u32x16_u __attribute__((address_space(4))) *slots_ptr;
    const u32x16_u pa = *(slots_ptr)(uintptr_t)(perm + tb * 32), pb = *(slots_ptr)(uintptr_t)(perm + tb * 32 + 16);
    uint32_t id[32];
#pragma unroll
    for (int x = 0; x < 32; ++x) {
        const uint32_t t = x < 16 ? pa[x] : pb[x - 16];
        const bool real = t != BS_NOCOL && j < N;             // padded registers/sketches: id 0 in both codings
        uint32_t w = real ? ids[(size_t)t * Npad + j] : 0u;
        if (SPLIT && real && !(w >> 31)) w = (w & BS_RANK_MASK) + colcnt[(size_t)t * BS_CC_STRIDE + (w >> BS_SPLIT_SHIFT)];
        id[x] = w;
    }
    uint32_t u = 0;                                    // the "unique" plane
#pragma unroll
    for (int x = 0; x < 32; ++x) u |= (id[x] >> UBIT) << x;
    // forms: BS_FORM_STREAM = what this GPU's pair kernel walks; BS_FORM_EXCHANGE = what ranks exchange -- written only
    // once somebody has asked for it (d2g_bitslice_export: 29 MB of stores per prepare at config 3 that a single GPU never reads)
    uint32_t *dst = planes + tb * (size_t)(nbits_cap + 1) * Nstride + jpos;
    const bool ex = forms & BS_FORM_EXCHANGE, st = forms & BS_FORM_STREAM;
    uint32_t *sdst = st ? stream + slot * 2 * Nstride + jpos : nullptr;
    for (int b = 0; b < nbits; ++b) {
        uint32_t w = 0;
#pragma unroll
        for (int x = 0; x < 32; ++x) w |= ((id[x] >> b) & 1u) << x;
        if (ex) dst[(size_t)b * Nstride] = w;          // row coding: unique = 0 (BS_UNIQ ids have zero low bits)
        if (st) {
            sdst[(size_t)(2 * b) * Nstride] = w;
            sdst[(size_t)(2 * b + 1) * Nstride] = w | u;   // column coding: unique = all ones
        }
    }
    // the 64 slack words behind position Npad of a plane are never read as sketches: in the exchanged form the first 32 of the unique
    // plane's carry D2 of the group's 32 register slots (what the sparse-tile path of a rank that only receives planes sizes its bit
    // sets with: sp_unpack_kernel)
    if (ex) {
        uint32_t uw = u;
        if (jpos >= Npad && jpos < Npad + 32) { const uint32_t t = perm[tb * 32 + (jpos - Npad)]; uw = t != BS_NOCOL ? colcnt[(size_t)t * BS_CC_STRIDE + 4] : 0u; }
        dst[(size_t)nbits_cap * Nstride] = uw;
    }
}
template <bool SPLIT, typename IdT = uint32_t>
__global__ __launch_bounds__(256) void bs_planes_kernel(BsPlanesArgs a) { bs_planes_body<SPLIT, IdT>(a, blockIdx.x, blockIdx.y); }

// plane stream of an operand that arrived in the exchanged form (the gathered operand of the multi-GPU path,
// d2g_cmp_set_from_planes_dev)
__global__ __launch_bounds__(256) void bs_derive_kernel(const uint32_t *__restrict__ planes, uint32_t *__restrict__ stream,
                                                        size_t Nstride, int nbits_cap, const uint32_t *__restrict__ meta, int tb0) {
    const size_t j = (size_t)blockIdx.x * 256 + threadIdx.x;
    const size_t tb = (size_t)tb0 + blockIdx.y;
    if (j >= Nstride) return;
    const int nbits = live_planes(meta, (int)tb);
    const uint32_t *src = planes + tb * (size_t)(nbits_cap + 1) * Nstride + j;
    uint32_t *sdst = stream + stream_slot(meta, (int)tb) * 2 * Nstride + j;
    const uint32_t u = j + BS_SLACK < Nstride ? src[(size_t)nbits_cap * Nstride] : 0u;     // the slack words of the unique plane carry D2 per slot, not sketches
    for (int b = 0; b < nbits; ++b) {
        const uint32_t w = src[(size_t)b * Nstride];
        sdst[(size_t)(2 * b) * Nstride] = w;
        sdst[(size_t)(2 * b + 1) * Nstride] = w | u;
    }
}

// ------------------------------------------------------------------ 3. the pair kernel
constexpr int BS_THREADS = 256;
constexpr int BS_CB = 256;                // columns per workgroup tile (all variants)

// v_bitop3_b32 truth table: src0 = 0xF0, src1 = 0xCC, src2 = 0xAA
constexpr unsigned BITOP3_C_OR_A_XOR_B = 0xAA | (0xF0 ^ 0xCC);   // mismatch accumulation

// (the pair kernel's tile shape, explained below: 16 rows per wave, JR 64-column groups per lane)
#ifndef D2G_BS_WPE
#define D2G_BS_WPE 7
#endif
#ifndef D2G_BS_JR
#define D2G_BS_JR 2
#endif
constexpr int BS_IW = 16;
constexpr int BS_JR = D2G_BS_JR;              // 64-column groups per lane: a wave owns 16 x (64*JR) pairs

__device__ __forceinline__ bool sp_dense_mode(const uint32_t *__restrict__ ctl, uint32_t cand);   // section 4
#include "d2g_k2_patch.h"

// IW = 16 rows per wave (one s_load_dwordx16 per plane), JR = 64-column groups per lane,
// WC = waves side by side along the columns (WC * JR * 64 = 256).  Per 32-register group: plane 0
// initialises z = r ^ c (no zeroing), planes 1.. accumulate with v_bitop3 z |= r ^ c, and one accumulating
// v_bcnt finishes the group: nbits + 1 VALU operations per pair and group.
//
// The kernel is bound by instruction ISSUE, all kinds counted: at 4, 5 or 6 waves per SIMD it takes the same
// time, and it got 13 % faster when the per-plane address arithmetic was (experimentally) constant-folded
// away -- scalar instructions are not free riders next to the vector ones.  Hence the plane STREAM: the
// live planes of all groups lie back to back (row words, then column words), the wave keeps ONE uniform
// pointer that advances by one block per plane, row words are an s_load_dwordx16 at the pointer and column
// words a global_load_dword at pointer + per-lane offset (saddr + voffset form: no vector address math).
// The operands of the next plane are requested before the current one is computed and land in the other
// of two explicitly alternating register sets.
//
// Epilogue: interior tiles (every pair of the wave's 16 x 64*JR block is wanted and off the diagonal --
// all but the ones on the triangle's edge) take a branch-free path: the row's output base is a scalar,
// the lane adds its column, so an output costs one table gather and one store.

template <int JR>
struct BsOperands {                         // the prefetched operands of one plane
    u32x16_u sa;                            // 16 row words (SGPRs)
    uint32_t vb[JR];                        // this lane's column words
};

// Scalar loads return out of order, so the only wait there is for them is lgkmcnt(0): it must come BEFORE
// the next s_load is issued -- left to the compiler it lands at the first use of the current operands,
// after the prefetch was issued, and the prefetch is then waited for on the spot.
template <int JR>
__device__ __forceinline__ BsOperands<JR> bs_fetch(const uint32_t *&ptr, uint32_t coff, size_t step) {
    __builtin_amdgcn_s_waitcnt(0xc07f);     // lgkmcnt(0): the operands about to be used have arrived
    __builtin_amdgcn_sched_barrier(0);
    BsOperands<JR> o;
    // constant address space: the operand is never written while this kernel runs, and a uniform address in
    // that space is always a scalar load (s_load_dwordx16), whatever the optimiser can or cannot prove
    typedef const u32x16_u __attribute__((address_space(4))) *row_words_ptr;
    o.sa = *(row_words_ptr)(uintptr_t)ptr;
    // the per-lane offset is laundered so that loop strength reduction cannot turn (uniform pointer + lane
    // offset) into a per-lane 64-bit running address: that costs a vector add per plane and four more VGPRs;
    // as written the loads select the saddr + voffset form
    uint32_t co = coff;
    asm volatile("" : "+v"(co));
#pragma unroll
    for (int c = 0; c < JR; ++c)
        o.vb[c] = *reinterpret_cast<const uint32_t *>(reinterpret_cast<const char *>(ptr) + co + 256 * c);
    ptr += step;
    return o;
}

template <int JR, bool FIRST>
__device__ __forceinline__ void bs_plane(const BsOperands<JR> &o, uint32_t (&z)[BS_IW][JR]) {
#pragma unroll
    for (int i = 0; i < BS_IW; ++i)
#pragma unroll
        for (int c = 0; c < JR; ++c)
            z[i][c] = FIRST ? (o.sa[i] ^ o.vb[c]) : __builtin_amdgcn_bitop3_b32(o.sa[i], o.vb[c], z[i][c], BITOP3_C_OR_A_XOR_B);
}

// one 32-register group with `nbits` id planes.  `a` holds plane 0 of this group on entry and plane 0 of the
// next group on exit (the stream has one block of slack after its last plane).  A copy between the two
// operand sets (8 s_mov_b64 + JR v_mov) happens at most once per GROUP, when the plane count is odd.
template <int JR>
__device__ __forceinline__ void bs_group(int nbits, const uint32_t *&ptr, uint32_t coff, size_t step, BsOperands<JR> &a,
                                         uint32_t (&acc)[BS_IW][JR]) {
    uint32_t z[BS_IW][JR];
    BsOperands<JR> b = bs_fetch<JR>(ptr, coff, step);
    bs_plane<JR, true>(a, z);                        // plane 0
    const int rest = nbits - 1;                      // planes 1 .. nbits-1, two per iteration (a counted loop: z stays in place)
    for (int k = rest >> 1; k > 0; --k) {
        a = bs_fetch<JR>(ptr, coff, step);
        bs_plane<JR, false>(b, z);                   // odd plane
        b = bs_fetch<JR>(ptr, coff, step);
        bs_plane<JR, false>(a, z);                   // even plane
    }
    if (rest & 1) {
        a = bs_fetch<JR>(ptr, coff, step);           // the next group's plane 0
        bs_plane<JR, false>(b, z);
    } else {
        a = b;                                       // b holds the next group's plane 0
    }
#pragma unroll
    for (int i = 0; i < BS_IW; ++i)
#pragma unroll
        for (int c = 0; c < JR; ++c) acc[i][c] += __builtin_popcount(z[i][c]);     // v_bcnt_u32_b32 acc, z, acc
}

template <int JR, class Store>
__global__ __launch_bounds__(BS_THREADS) __attribute__((amdgpu_waves_per_eu(D2G_BS_WPE))) void k2_bitslice_kernel(
    const uint32_t *__restrict__ stream, size_t Nstride, const uint32_t *__restrict__ meta, int ntb, uint32_t S, PairShape sh, Store store,
    const uint32_t *__restrict__ gate, uint32_t gate_cand, SpPatchArgs pa) {
    constexpr int IW = BS_IW;
    constexpr int WC = BS_CB / (64 * JR);          // waves along columns: 2 (JR=2)
    constexpr int WR = 4 / WC;                     // waves along rows
    constexpr int RB = WR * IW;                    // rows per workgroup tile
    if (gate && !sp_dense_mode(gate, gate_cand)) {           // launched behind the sparse path: the tile walk only when that decided for the dense walk;
        sp_patch_lut(pa, sh, store, S, (size_t)blockIdx.x * BS_THREADS + threadIdx.x, (size_t)gridDim.x * BS_THREADS);   // otherwise a short pair list's table epilogue
        return;
    }
    unsigned ct, rt;
    if (!tile_of_block(sh, blockIdx.x, ct, rt)) return;      // XCD-balanced, column-major wanted tiles
    const size_t i0 = sh.i_lo + (size_t)rt * RB;
    const size_t jt0 = (size_t)(sh.ct0 + ct) * BS_CB;

    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    const size_t iw0 = i0 + (size_t)(wave / WC) * IW;
    const size_t j0 = jt0 + (size_t)(wave % WC) * (64 * JR);
    if (iw0 >= sh.i_hi) return;
    if (sh.ut && j0 + 64 * JR - 1 <= iw0) return;

    uint32_t acc[IW][JR];
#pragma unroll
    for (int i = 0; i < IW; ++i)
#pragma unroll
        for (int c = 0; c < JR; ++c) acc[i][c] = 0;

    // one uniform pointer: the wave's 16 row words of the current plane; its column words sit at a fixed
    // per-lane byte offset from it (Nstride >= Npad + 64 > iw0, so the offset is positive and < 2^32)
    const uint32_t *ptr = stream + iw0;
    const uint32_t coff = (uint32_t)(Nstride - iw0 + j0 + (size_t)lane) * 4u;
    const size_t step = 2 * Nstride;                             // words per plane block (row words + column words)

    BsOperands<JR> nx = bs_fetch<JR>(ptr, coff, step);           // group 0, plane 0
    int nbits_nx = live_planes(meta, 0);
    for (int tb = 0; tb < ntb; ++tb) {
        const int nbits = nbits_nx;                              // uniform, per 32-register group
        nbits_nx = live_planes(meta, tb + 1 < ntb ? tb + 1 : 0); // scalar load, one group ahead
        bs_group<JR>(nbits, ptr, coff, step, nx, acc);
    }

    // interior: all 16 rows and all 64*JR columns of this wave are wanted pairs off the diagonal
    const bool interior = iw0 + IW <= sh.i_hi && j0 >= sh.j_lo && j0 + 64 * JR <= sh.j_hi &&
                          (sh.ut ? j0 > iw0 + IW - 1 : (j0 > iw0 + IW - 1 || j0 + 64 * JR <= iw0));
    if (interior) {
        uint32_t val[IW][JR];
#pragma unroll
        for (int i = 0; i < IW; ++i)
#pragma unroll
            for (int c = 0; c < JR; ++c) val[i][c] = store.value_from_mismatches(S, acc[i][c]);
        const uint32_t jl = (uint32_t)j0 + (uint32_t)lane;       // < 2^30
#pragma unroll
        for (int i = 0; i < IW; ++i) {
            const size_t rb = out_row_base(sh, iw0 + i);         // uniform: out_pos(ii, jj) = rb + jj
#pragma unroll
            for (int c = 0; c < JR; ++c) store.put_row(rb, jl + 64u * c, val[i][c]);
        }
        return;
    }
    // edge tiles.  Padded registers never mismatch; a sketch equals itself even where its values are
    // column-unique (the two codings of "unique" only separate DIFFERENT sketches)
    uint32_t val[IW][JR];
#pragma unroll
    for (int i = 0; i < IW; ++i)
#pragma unroll
        for (int c = 0; c < JR; ++c)
            val[i][c] = store.value((iw0 + i) == (j0 + lane + 64 * c) ? S : S - acc[i][c]);
#pragma unroll
    for (int i = 0; i < IW; ++i) {
        const size_t ii = iw0 + i;
        if (ii >= sh.i_hi) break;
#pragma unroll
        for (int c = 0; c < JR; ++c) {
            const size_t jj = j0 + lane + 64 * c;
            if (jj < sh.j_hi && jj >= sh.j_lo && (!sh.ut || jj > ii)) store.put(out_pos(sh, ii, jj), val[i][c]);
        }
    }
}

#include "d2g_k2_sparse.h"

// gathered (caller-owned) operands carry the row coding + the unique plane only: derive the column coding.
// Done before EVERY launch on such a set -- the library cannot know when the caller re-gathered into the
// buffer, and the pass is ~2 % of the pair kernel it precedes.
int refresh_borrowed(d2g_ctx *ctx, const d2g_cmp_set *set, hipStream_t s) {
    if (!set->borrowed || set->managed) return D2G_OK;       // managed: the engine derived the stream as the groups arrived
    return d2g_bitslice_derive_groups(ctx, set, 0, set->ntb, s);
}


template <class Store>
int launch_bitslice(d2g_ctx *ctx, const d2g_cmp_set *set, PairShape sh, Store store, hipStream_t s) {
    if (int rc = finish_shape(ctx, sh, BS_JR == 2 ? 32u : 64u)) return rc;   // workgroup tile = (16 * JR) rows x 256 columns (4 waves of 16 x 64*JR)
    if (sh.nvalid_total == 0) return D2G_OK;
    if (int rc = refresh_borrowed(ctx, set, s)) return rc;
    if (int rc = d2g_bitslice_ensure_natural(ctx, set, s)) return rc;
    d2g_timer tm(ctx, &ctx->ev_k2, s);
    hipLaunchKernelGGL((k2_bitslice_kernel<BS_JR, Store>), dim3(sh.per_xcd * 8), dim3(BS_THREADS), 0, s, set->d_stream,
                       set->Nstride, set->d_meta, set->ntb, (uint32_t)set->S, sh, store, (const uint32_t *)nullptr, 0u, SpPatchArgs{});
    tm.stop();
    D2G_HIP(ctx, hipGetLastError());
    return D2G_OK;
}

}  // namespace

// geometry of the bit-sliced operand: a function of N (and S) only, identical on every rank.
// A column holds at most floor(N/2) values that occur twice; ranks 1..D2 plus the two codes of "unique"
// (0 and 2^nbits - 1) need 2^nbits >= D2 + 2.
void d2g_bitslice_geometry(d2g_cmp_set *set) {
    set->nbits_cap = 1;
    while ((1ull << set->nbits_cap) < set->N / 2 + 2) ++set->nbits_cap;
    set->ntb = (int)div_up<size_t>(set->S, 32);
    set->Nstride = set->Npad + BS_SLACK;
}

// the plane stream: at most nbits_cap live planes per group, two codings each, + one block of slack (the
// kernel's prefetch runs one plane past the end)
int d2g_bitslice_alloc_stream(d2g_ctx *ctx, d2g_cmp_set *set) {
    return set->d_stream.alloc(ctx, ((size_t)set->ntb * set->nbits_cap + 1) * 2 * set->Nstride, "bitslice alloc");
}

namespace {
// workspace every preparing set needs (ids, per-column counts, column plan, meta + status); the rank kernel's hash space
int alloc_prepare_workspace(d2g_ctx *ctx, d2g_cmp_set *set) {
    const size_t N = set->N, S = set->S, Npad = set->Npad;
    if (N >= (1ull << 30)) { ctx->last_error = "bitslice: N too large"; return D2G_ERR_UNSUPPORTED; }
    d2g_bitslice_geometry(set);
    // hash space: power of two >= 1.5 N (load <= 2/3), at least 64 slots; walked in LDS-sized partitions
    set->T = 64; set->logT = 6;
    while ((uint64_t)set->T * 2 < (uint64_t)N * 3) { set->T <<= 1; ++set->logT; }
    // narrow slices of large N: several workgroups per column (each walks its share of the hash partitions) until the CUs are covered
    set->nsplit = 1;
    if (set->logT > BS_LOG_TLDS_MAX && N < (1ull << BS_SPLIT_SHIFT)) {
        const uint32_t nparts = set->T >> BS_LOG_TLDS_MAX;
        int want = 1;
        while (want < 4 && (uint32_t)want * 2 <= nparts && S * (size_t)want < (size_t)std::max(ctx->num_cus, 1)) want *= 2;
        if (ctx->k2.nsplit_req && (uint32_t)ctx->k2.nsplit_req <= nparts) want = ctx->k2.nsplit_req;   // D2G_BS_NSPLIT (tests / experiments)
        set->nsplit = want;
    }
    const char *what = "bitslice alloc";
    int rc;
    // the ids of a set whose rank kernel is single-partition are 16-bit words (BsId): decided HERE, once per set, and every kernel that touches them follows
    set->id_bits = (ctx->k2.id16 && set->logT <= BS_LOG_TLDS_MAX) ? 16 : 32;
    D2G_CHECK(ctx, set->id_bits == 32 || (N <= BS_ID16_MAX_N && set->nsplit == 1), "bitslice: 16-bit ids need a single-partition rank kernel");
    const size_t id_words = set->id_bits == 16 ? (S * Npad + 1) / 2 : S * Npad;
    if ((rc = set->d_ids.alloc(ctx, id_words, what)) ||
        (rc = d2g_hip_status(ctx, hipMemset(set->d_ids, 0, id_words * sizeof(uint32_t)), what)) ||     // split rank passes rely on "no stale pending word"; the link passes and emit on "the padding holds id 0"
        (rc = set->d_colcnt.alloc(ctx, S * BS_CC_STRIDE, what)) ||
        (rc = set->d_perm.alloc(ctx, (size_t)set->ntb * 32, what)) ||
        (rc = set->own_meta.alloc(ctx, (size_t)(set->ntb + 4), what)) ||
        (rc = d2g_hip_status(ctx, hipMemset(set->own_meta, 0, (size_t)(set->ntb + 4) * sizeof(uint32_t)), what))) return rc;
    set->d_meta = set->own_meta;
    return D2G_OK;
}
// the bit transpose of the ids (bs_planes_kernel): the plane stream and / or the exchange form (`forms`; the latter into `planes`)
int launch_planes(d2g_ctx *ctx, const d2g_cmp_set *set, uint32_t *planes, int forms, hipStream_t s) {
    const dim3 grid((unsigned)div_up<size_t>(set->Nstride, 256), (unsigned)set->ntb);
    const bool split = set->logT > BS_LOG_TLDS_MAX && set->nsplit > 1;
    D2G_CHECK(ctx, !(split && set->id_bits == 16), "bitslice: a split set with 16-bit ids");
    hipLaunchKernelGGL((set->id_bits == 16 ? bs_planes_kernel<false, uint16_t> : split ? bs_planes_kernel<true> : bs_planes_kernel<false>), grid, dim3(256), 0, s, planes_args_of(set, planes, forms));
    D2G_HIP(ctx, hipGetLastError());
    return D2G_OK;
}
// once armed: `s` waits for `ev` when the scope ends, however it ends
struct JoinOnExit {
    hipStream_t s; hipEvent_t ev = nullptr;
    ~JoinOnExit() { if (ev) (void)hipStreamWaitEvent(s, ev, 0); }
};
}  // namespace

// one-time allocation of the bit-sliced operand and its workspace
int d2g_bitslice_alloc(d2g_ctx *ctx, d2g_cmp_set *set) {
    if (int rc = alloc_prepare_workspace(ctx, set)) return rc;
    if (int rc = set->own_planes.alloc(ctx, (size_t)set->ntb * (set->nbits_cap + 1) * set->Nstride, "bitslice alloc")) return rc;
    set->d_planes = set->own_planes;
    if (int rc = d2g_bitslice_alloc_stream(ctx, set)) return rc;
    set->ncols = set->S;
    if (sparse_enabled(ctx, set->N) && set->S < 65536 && sp_alloc(ctx, set) != D2G_OK) (void)hipGetLastError();   // (S: the sparse kernel packs two mismatch counts into one LDS word)
    if (set->sparse_ok() && set->nsplit == 1) {                          // one holder per shared value, left by the rank kernel (sp_olink_kernel)
        set->sp->owner_stride = set->N / 2 + 8;
        if (set->sp->d_owner.alloc(ctx, set->S * set->sp->owner_stride, "bitslice owner alloc") != D2G_OK) (void)hipGetLastError();
    }   // no memory for the sparse path's buffers: the dense walk works without them
    return D2G_OK;
}

// ids + column plan + planes for the operand currently in set->d_cols.  Fully asynchronous on `s`.
// meta[0..ntb) = per-group shared-value counts; meta[ntb] = status word (bit 0: the rank kernel's LDS table
// overflowed on some column -- see d2g_bitslice_status)
int d2g_bitslice_prepare(d2g_ctx *ctx, d2g_cmp_set *set, hipStream_t s) {
    const size_t N = set->N, S = set->S, Npad = set->Npad;
    SpState *const sp = set->sp.get();
    // an announced output (d2g_cmp_ut_announce_dev): this prepare's latency-bound kernels carry its fill -- unless the ordering is going to
    // be skipped (the remembered give-up: the launch will be dense and fill nothing)
    const bool sparse_path = sp && !set->export_only && !set->want_exchange;
    JoinOnExit join{s};
    if (sp) {
        // (the remembered word is device-written host memory read without synchronisation: read ONCE per prepare -- ADVICE r5 -- and handed down)
        sp->dec.skip_cached = sparse_path ? (sp_will_skip(ctx, *sp) ? 1 : 0) : -1;
        sp->announced.begin(ctx->k2.ride, sparse_path && sp->dec.skip_cached != 1);
        const size_t pieces = sp->announced.out ? sp_fill_pieces(sp->announced.cnt) : 0;
        sp->dec.fill_announced = pieces; sp->dec.fill_rank = sp->dec.fill_carried = 0;   // (diagnostics: d2g_cmp_set_fill_detail)
    }
    if (sp && sp->announced.riding() >= SP_SIDE_FILL_PIECES) {
        if (!sp->fill_stream) {
            if (sp->fill_stream.create(hipStreamNonBlocking) != hipSuccess || sp->fill_fork.create(hipEventDisableTiming) != hipSuccess ||
                sp->fill_join.create(hipEventDisableTiming) != hipSuccess) { (void)hipGetLastError(); sp->fill_stream.reset(); sp->fill_fork.reset(); sp->fill_join.reset(); }
        }
        if (sp->fill_stream) {
            // behind everything already on `s` (the transpose of this update; whoever read the output last), beside everything this prepare enqueues
            hipStream_t fs = sp->fill_stream;
            D2G_HIP(ctx, hipEventRecord(sp->fill_fork, s));
            D2G_HIP(ctx, hipStreamWaitEvent(fs, sp->fill_fork, 0));
            // from here on every return, failed or not, joins the fill back into `s`: the launch writes into the filled output, and after an
            // error the caller must not find a fill still writing into its buffer, unordered with what it does next
            join.ev = sp->fill_join;
            const uint32_t pieces = sp->announced.riding();
            const SpRider all = sp->announced.take_all();                // nothing left for the riders
            const unsigned fgrid = sp_side_fill_grid(ctx, pieces, all.cnt, N, S);
            hipLaunchKernelGGL(sp_side_fill_kernel, dim3(fgrid), dim3(256), 0, fs, all, pieces);
            D2G_HIP(ctx, hipEventRecord(sp->fill_join, fs));
        }
    }
    // the status word meta[ntb] was zeroed by the transpose kernel that filled d_cols (no memset node in the chain)
    const bool multi = set->logT > BS_LOG_TLDS_MAX;
    const int nsplit = multi ? set->nsplit : 1;
    {
        const int logTl = set->logT < BS_LOG_TLDS_MAX ? set->logT : BS_LOG_TLDS_MAX;
        const size_t lds = (size_t(1) << logTl) * sizeof(uint32_t);
        const bool id16 = set->id_bits == 16;
        D2G_CHECK(ctx, !(multi && id16), "bitslice: the multi-partition rank kernel with 16-bit ids");
        void (*kern)(const uint64_t *, size_t, size_t, uint32_t, int, void *, uint32_t *, uint32_t *, int, uint32_t, int, uint32_t *, size_t, SpRider, uint32_t) = bs_rank_kernel<false, false>;
        const bool fast = !multi && N <= (size_t)BS_RANK_PF * BS_RANK_THREADS;
        if (multi) kern = bs_rank_kernel<true, false>;
        else if (fast) kern = id16 ? bs_rank_kernel<false, true, uint16_t> : bs_rank_kernel<false, true>;
        else if (id16) kern = bs_rank_kernel<false, false, uint16_t>;
        if (lds > 48 * 1024)
            D2G_HIP(ctx, hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        // split passes tell their pending words from final ids by a tag and trust that ids[] holds nothing else that looks pending.  A
        // prepare that overflowed (status bit 0) may leave pending words behind, and the multi-GPU engine re-uses its exporter sets step
        // after step: ids[] starts from zero in every split prepare -- a few MB for the narrow column slices that are split
        if (nsplit > 1) D2G_HIP(ctx, hipMemsetAsync(set->d_ids, 0, S * Npad * sizeof(uint32_t), s));
        // a set's first prepare looks at its matrix before it orders it (below); asked HERE, once, because the rank kernel's share of an announced fill
        // depends on it too
        const bool look = sparse_path && sp_sample_due(ctx, set);
        // the FAST rank kernel writes the first pieces of an announced fill itself (D2G_SP_RANK_SHARE) -- when this prepare's path is known as it is enqueued: a
        // first look may still decide for the dense walk, whose launch fills nothing (a remembered give-up carries nothing at all: announced.begin), and
        // a large output has its side stream (taken above: nothing is left here)
        SpRider rank_fill = SP_NO_RIDER; uint32_t rank_n = 0;
        if (sparse_path && fast && !look && sp->announced.riding() < SP_SIDE_FILL_PIECES)
            rank_fill = sp->announced.take_first((unsigned)ctx->k2.rank_share, (uint64_t)SP_RANK_FILL_PER_WG * S, &rank_n);
        D2G_CHECK(ctx, rank_n <= (uint64_t)SP_RANK_FILL_PER_WG * S * nsplit, "bitslice: the rank kernel's share of the fill does not fit its grid");
        if (sp) sp->dec.fill_rank = rank_n;
        hipLaunchKernelGGL(kern, dim3((unsigned)(S * nsplit)), dim3(BS_RANK_THREADS), lds, s, set->d_cols, N, Npad, set->T, set->logT,
                           (void *)set->d_ids.get(), set->d_colcnt, set->d_meta + set->ntb, ctx->k2.tagbits_max, (uint32_t)S, nsplit,
                           (sp && nsplit == 1) ? sp->d_owner.get() : (uint32_t *)nullptr, sp ? sp->owner_stride : 0, rank_fill, rank_n);
        if (sp) sp->dec.kernels = 2 + (join.ev ? 1 : 0);               // the transpose in front of this prepare, the rank kernel (, the side fill)
        // the first look: the sample needs the ids only, so it stands HERE and the two kernels below run while the host waits for its word
        // (sp_sample_collect)
        if (look) { if (int rc = sp_sample_enqueue(ctx, set, s)) return rc; if (sp->dec.sample_pending) sp->dec.kernels += 2; }
        // Three schedules from here on.  Behind the rank kernel the chain A = column plan -> planes (reads colcnt and ids; writes perm, meta, the caller's-order
        // stream) and the chain B = the ordering (link pass 0 -> flatten -> link pass 1 -> count -> attach -> scan -> place -> emit: reads ids, owner, labels;
        // writes labels, hints, counts, sperm / sinv, tile bitmap, list) meet only in sp_permute.
        //   classic   A in front of B, kernel by kernel: rank, plan, planes, link 0, flatten, link 1, count, attach, scan, place, emit, permute
        //   merged    A inside launches of B (sp_launch_merged):   rank, [plan + link 0], [flatten + planes], link 1, count, attach, scan, place, emit, permute
        //             (two launches and ~9 us fewer per step at config 3: profiles/k2_merged_prepare.txt)
        //   merged 2  the planes, which nobody reads before sp_permute, leave the ordering's critical path: they stand BEHIND the pair-list kernel's workgroups,
        //             whose clean columns are done after half the launch (sp_emit_kernel<IdT, true>):
        //                                                          rank, [plan + link 0], flatten, link 1, count, attach, scan, place, [emit + planes], permute
        //             (profiles/k2_planes_emit.txt)
        // The merged ones need the streaming link form on unsplit columns, and a prepare whose path is known when it is enqueued: the first prepare of a set and
        // the retry of a remembered give-up decide between dense and sparse on the host BEHIND the rank kernel (the first look) -- link pass 0 must not be
        // enqueued before that -- and a remembered give-up runs no ordering at all.  Exporter and exchange sets have no ordering.  D2G_K2_MERGE=0: classic.
        const int merged = (sparse_path && !look && ctx->k2.merge && nsplit == 1 && sp->d_owner && ctx->k2.olink && ctx->k2.link && sp->dec.skip_cached != 1) ? ctx->k2.merge : 0;
        if (sp) sp->dec.merged = merged;
        if (!merged) {
            unsigned g = 1; const SpRider rd = sp ? sp->announced.take(1, SP_RW_PLAN, false, 1, &g) : SP_NO_RIDER;
            const BsPlanArgs pa{set->d_colcnt, (uint32_t)S, set->ntb, nsplit, set->d_perm, set->d_meta, set->d_meta + set->ntb, set->ex_meta, set->ex_status, ctx->k2.sort ? 1 : 0};
            hipLaunchKernelGGL(bs_colplan_kernel, dim3(g), dim3(BS_PLAN_THREADS), bs_plan_lds_words((uint32_t)set->ntb * 32u, pa.sort) * 4, s, pa, rd);
            if (sp) sp->dec.kernels += 1;
        }
    }
    if (sparse_path) {
        // sparse path (section 4): the caller's-order stream (the dense walk and rectangular launches read it), the families, the pair list and
        // the stream in family order
        // (gathering the ids through d_sperm inside bs_planes_kernel was measured: 74 us instead of 18 at config 3 -- 1024 columns of
        // uncoalesced 4-byte loads; permuting the finished stream touches 256 rows of words and leaves the caller's-order stream valid)
        // (a second queue for the caller's-order planes beside the ordering, and for the fill beside the tile list, was measured in round 4:
        // the kernels slow each other down by what the overlap hides and the events cost more: dropped)
        // (the ordering's arrays and the tile bitmap were initialised by the transpose in front of this prepare: no launch / memset of their own)
        if (!sp->dec.merged) { if (int rc = launch_planes(ctx, set, set->d_planes, BS_FORM_STREAM, s)) return rc; sp->dec.kernels += 1; }
        if (int rc = sp_sample_collect(ctx, set, s)) return rc;         // (the first look, enqueued behind the rank kernel: the host waits for its word here)
        if (int rc = sp_prepare_order(ctx, set, nsplit > 1, s)) return rc;
        if (int rc = sp_permute(ctx, set, s)) return rc;
        set->srt_valid = true; set->nat_valid = true;
        sp->dec.fill_carried = sp->announced.next - sp->dec.fill_rank;
        if (sp->announced.riding()) sp->filled.set_by_riders(sp->announced);
        else sp->filled.void_after_prepare();
        sp->announced.served();
        D2G_HIP(ctx, hipGetLastError());
        return D2G_OK;
    }
    if (sp) sp->announced.served();
    const int forms = set->export_only ? BS_FORM_EXCHANGE : (BS_FORM_STREAM | (set->want_exchange ? BS_FORM_EXCHANGE : 0));
    if (int rc = launch_planes(ctx, set, set->export_only ? set->ex_planes : set->d_planes, forms, s)) return rc;
    if (sp) sp->dec.kernels += 1;
    set->srt_valid = false; set->nat_valid = true;
    return D2G_OK;
}

SpInit d2g_bitslice_sp_init(const d2g_cmp_set *set) { return sp_init_of(set); }

// the caller's-order stream of a set whose last prepare only wrote the sorted one (rectangular launches, exports)
int d2g_bitslice_ensure_natural(d2g_ctx *ctx, const d2g_cmp_set *set, hipStream_t s) {
    if (set->nat_valid || set->borrowed || set->export_only) return D2G_OK;
    if (int rc = launch_planes(ctx, set, set->d_planes, BS_FORM_STREAM, s)) return rc;
    set->nat_valid = true;
    return D2G_OK;
}

// the exchange form of the operand last prepared: written from the ids on first request, by every prepare afterwards
int d2g_bitslice_export(d2g_ctx *ctx, d2g_cmp_set *set, hipStream_t s) {
    if (set->borrowed || set->want_exchange || set->export_only) return D2G_OK;
    set->want_exchange = true;
    return launch_planes(ctx, set, set->d_planes, BS_FORM_EXCHANGE, s);
}

// ---- exporter sets: the multi-GPU engine's per-rank column slices (d2g_mgpu.hip)
int d2g_bitslice_exporter_create(d2g_ctx *ctx, size_t N, size_t S_local, d2g_cmp_set **out) {
    *out = nullptr;
    d2g_cmp_set *set = new (std::nothrow) d2g_cmp_set();
    if (!set) return D2G_ERR_NOMEM;
    set->ctx = ctx; set->N = N; set->S = S_local;
    set->Npad = div_up<size_t>(N, BS_CB) * BS_CB;
    set->algo = D2G_CMP_BITSLICE;
    set->export_only = true;
    if (int rc = set->d_cols.alloc(ctx, set->Npad * S_local, "bitslice exporter alloc")) { delete set; return rc; }
    if (int rc = alloc_prepare_workspace(ctx, set)) { delete set; return rc; }
    *out = set;
    return D2G_OK;
}
void d2g_bitslice_set_export_target(d2g_cmp_set *set, uint32_t *planes, uint32_t *meta, uint32_t *status) {
    set->ex_planes = planes; set->ex_meta = meta; set->ex_status = status;
}

int d2g_bitslice_derive_groups(d2g_ctx *ctx, const d2g_cmp_set *set, int g0, int g1, hipStream_t s) {
    if (g1 <= g0) return D2G_OK;
    dim3 grid((unsigned)div_up<size_t>(set->Nstride, 256), (unsigned)(g1 - g0));
    hipLaunchKernelGGL(bs_derive_kernel, grid, dim3(256), 0, s, set->d_planes, set->d_stream, set->Nstride, set->nbits_cap, set->d_meta, g0);
    D2G_HIP(ctx, hipGetLastError());
    return D2G_OK;
}

// synchronises `s`; D2G_ERR_INTERNAL when the last prepare overflowed its hash partitions
int d2g_bitslice_status(d2g_ctx *ctx, const d2g_cmp_set *set, hipStream_t s) {
    uint32_t st = 0;
    if (set->borrowed) {
        // a gathered operand has no status word of its own; the multi-GPU engine's carries one per preparing rank and chunk
        if (!set->status_words || set->n_status <= 0) { D2G_HIP(ctx, hipStreamSynchronize(s)); return D2G_OK; }
        std::vector<uint32_t> w((size_t)set->n_status);
        D2G_HIP(ctx, hipMemcpyAsync(w.data(), set->status_words, w.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
        D2G_HIP(ctx, hipStreamSynchronize(s));
        for (uint32_t x : w) st |= x;
    } else {
        D2G_HIP(ctx, hipMemcpyAsync(&st, set->d_meta + set->ntb, sizeof(st), hipMemcpyDeviceToHost, s));
        D2G_HIP(ctx, hipStreamSynchronize(s));
    }
    if (st & 1u) {
        ctx->last_error = "bitslice prepare: a register column put more distinct values into one hash partition than its LDS table holds "
                          "(adversarial / extremely skewed column); use D2G_CMP_DIRECT for this matrix";
        return D2G_ERR_INTERNAL;
    }
    return D2G_OK;
}

int d2g_bitslice_ut(d2g_ctx *ctx, const d2g_cmp_set *set, size_t r0, size_t r1, uint32_t *eq_out, const float *lut,
                    float *fout, hipStream_t s) {
    const PairShape sh = ut_shape(set->N, r0, r1);
    if (set->srt_valid) {
        if (eq_out) return launch_sparse(ctx, set, sh, StoreEq{eq_out}, eq_out, s);
        return launch_sparse(ctx, set, sh, StoreLut{fout, lut}, reinterpret_cast<uint32_t *>(fout), s);
    }
    if (set->sp) set->sp->filled.clear();                              // (an early fill is void once a launch has written every output itself)
    if (eq_out) return launch_bitslice(ctx, set, sh, StoreEq{eq_out}, s);
    return launch_bitslice(ctx, set, sh, StoreLut{fout, lut}, s);
}

int d2g_bitslice_prefill(d2g_ctx *ctx, d2g_cmp_set *set, size_t r0, size_t r1, uint32_t *eq_out, const float *lut, float *fout, hipStream_t s) {
    if (eq_out) return sp_prefill(ctx, set, r0, r1, StoreEq{eq_out}, eq_out, s);
    return sp_prefill(ctx, set, r0, r1, StoreLut{fout, lut}, reinterpret_cast<uint32_t *>(fout), s);
}

int d2g_bitslice_announce(d2g_ctx *, d2g_cmp_set *set, size_t r0, size_t r1, uint32_t *eq_out, const float *lut, float *fout) {
    const size_t cnt = d2g_ut_count(set->N, r0, r1);
    if (!set->sp) return D2G_OK;
    SpAnnounced &an = set->sp->announced;
    an.cancel();
    if (!cnt || (!eq_out && !fout)) return D2G_OK;                     // the cancelling form: nothing rides on the next prepare
    if (eq_out) an.announce(eq_out, cnt, nullptr);
    else an.announce(reinterpret_cast<uint32_t *>(fout), cnt, reinterpret_cast<const uint32_t *>(lut));
    return D2G_OK;
}

int d2g_bitslice_rect(d2g_ctx *ctx, const d2g_cmp_set *set, size_t a0, size_t a1, size_t b0, size_t b1, uint32_t *eq_out,
                      hipStream_t s) {
    return launch_bitslice(ctx, set, rect_shape(set->N, a0, a1, b0, b1), StoreEq{eq_out}, s);
}

// ---- sparse tiles on the multi-GPU engine's gathered operand (replicated: every rank orders and marks the whole operand itself --
// the pair phase of a block-structured matrix shrinks by the fraction of tiles listed, the fixed costs stay per rank)
int d2g_bitslice_managed_sparse_alloc(d2g_ctx *ctx, d2g_cmp_set *set) {
    if (!set->borrowed || set->sparse_ok()) return D2G_OK;
    set->ncols = (size_t)set->ntb * 32;
    if (!(sparse_enabled(ctx, set->N) && set->S < 65536)) return D2G_OK;
    const char *what = "bitslice sparse alloc";
    if (set->d_ids.alloc(ctx, set->ncols * set->Npad, what) != D2G_OK ||
        set->d_colcnt.alloc(ctx, set->ncols * BS_CC_STRIDE, what) != D2G_OK ||
        hipMemset(set->d_colcnt, 0, set->ncols * BS_CC_STRIDE * sizeof(uint32_t)) != hipSuccess) {
        // not enough memory for the sparse path's buffers: the dense walk works without them
        set->d_ids.reset(); set->d_colcnt.reset();
        (void)hipGetLastError();
        return D2G_OK;
    }
    if (sp_alloc(ctx, set) != D2G_OK) (void)hipGetLastError();
    return D2G_OK;
}

int d2g_bitslice_managed_ready(d2g_ctx *ctx, d2g_cmp_set *set, hipStream_t s) {
    if (!set->borrowed || !set->sparse_ok()) return D2G_OK;
    dim3 grid((unsigned)div_up<size_t>(set->Npad, 256), (unsigned)set->ntb);
    set->sp->dec.merged = 0; set->sp->dec.kernels = 1;            // (diagnostics: the unpack kernel, then the classic chain)
    hipLaunchKernelGGL(sp_unpack_kernel, grid, dim3(256), 0, s, set->d_planes, set->Nstride, set->nbits_cap, set->d_meta, set->N, set->Npad, set->d_ids, set->d_colcnt, sp_init_of(set));
    if (int rc = sp_prepare_order(ctx, set, false, s)) return rc;
    if (int rc = sp_permute(ctx, set, s)) return rc;
    D2G_HIP(ctx, hipGetLastError());
    set->srt_valid = true;
    return D2G_OK;
}

// the set's remembered decisions forgotten: its next prepare decides as a new set's first prepare does (measurements: bench.py's first_step_ms)
void d2g_bitslice_forget(d2g_cmp_set *set) {
    if (!set->sp) return;
    if (set->sp->h_gaveup) { set->sp->h_gaveup[SP_MW_GAVEUP] = 0; set->sp->h_gaveup[SP_MW_LIST_LEN] = 0; }
    set->sp->dec.prepares = 0; set->sp->dec.pred_valid = false;
}

// diagnostics of the sparse path's LAST launch on this set (synchronises `s`): see d2g.h
int d2g_bitslice_sparse_info(d2g_ctx *ctx, const d2g_cmp_set *set, hipStream_t s, uint32_t *out4) {
    out4[0] = out4[1] = out4[2] = out4[3] = 0;
    if (!set->srt_valid || !set->sp) { D2G_HIP(ctx, hipStreamSynchronize(s)); return D2G_OK; }
    const SpState &sp = *set->sp;
    uint32_t c[4] = {0, 0, 0, 0}, ord[4] = {0, 0, 0, 0}, pl = 0;
    if (!sp.last_ctl) { D2G_HIP(ctx, hipStreamSynchronize(s)); out4[0] = 1; return D2G_OK; }   // prepared, never launched
    D2G_HIP(ctx, hipMemcpyAsync(c, sp.last_ctl, sizeof c, hipMemcpyDeviceToHost, s));   // the control words the last launch used
    D2G_HIP(ctx, hipMemcpyAsync(ord, sp.d_order, sizeof ord, hipMemcpyDeviceToHost, s));
    D2G_HIP(ctx, hipMemcpyAsync(&pl, sp.d_plctl, sizeof pl, hipMemcpyDeviceToHost, s));
    D2G_HIP(ctx, hipStreamSynchronize(s));
    const bool dense = (c[1] & 1u) || (size_t)c[0] * 5 > (size_t)c[3] * 2;
    // [2]: bit 0 the prepare decided for the dense walk, bit 1 the dense kernel ran, bit 2 tiles + pair list were used, bit 3 the caller's order was kept,
    //      bit 4 the last prepare skipped the ordering (the one before had given up: sp_prepare_order)
    out4[0] = 1; out4[1] = c[0]; out4[2] = (ord[0] ? 1u : 0u) | (dense ? 2u : 4u) | (ord[0] ? 8u : 0u) | (sp.dec.skipped ? 16u : 0u);
    out4[3] = ord[0] ? 0u : (uint32_t)std::min<size_t>(pl, sp.plist_cap);
    return D2G_OK;
}

// diagnostics of the last prepare's first look and list form (synchronises `s`): see d2g.h
int d2g_bitslice_sparse_detail(d2g_ctx *ctx, const d2g_cmp_set *set, hipStream_t s, uint64_t *out8) {   // (out8: ten words)
    uint32_t binned = 0;
    if (set->sp) D2G_HIP(ctx, hipMemcpyAsync(&binned, set->sp->d_plctl + SP_PL_BINNED, 4, hipMemcpyDeviceToHost, s));   // (raised by sp_bin_kernel when the binned form ran)
    D2G_HIP(ctx, hipStreamSynchronize(s));
    if (!set->sp) return D2G_OK;
    const SpState &sp = *set->sp;
    out8[0] = sp.dec.looked ? 1 : 0; out8[1] = sp.dec.looked_dense ? 1 : 0;
    if (sp.dec.looked) for (int x = 0; x < 4; ++x) out8[2 + x] = sp.dec.samp_sums[x];   // (a prepare that did not look reports no sums: those of an earlier look are not its own)
    out8[6] = binned ? 1 : 0; out8[7] = sp.bin_cshift;
    out8[8] = (uint64_t)sp.dec.merged; out8[9] = sp.dec.kernels;
    return D2G_OK;
}

// what became of the output announced to the last prepare, in 32 KB pieces: announced, written by the rank kernel, by the prepare's other kernels (the
// riders; the side fill of a large output), left to the launch.  Host bookkeeping: nothing is synchronised
void d2g_bitslice_fill_detail(const d2g_cmp_set *set, uint64_t *out4) {
    out4[0] = out4[1] = out4[2] = out4[3] = 0;
    if (!set->sp) return;
    const SpDecision &d = set->sp->dec;
    out4[0] = d.fill_announced; out4[1] = d.fill_rank; out4[2] = d.fill_carried; out4[3] = d.fill_announced - d.fill_rank - d.fill_carried;
}

int d2g_sparse_bin_geometry(size_t N, uint32_t *cshift, uint32_t *nch, uint32_t *nbins, int *binned_ok) {
    if (!N) return D2G_ERR_INVALID;
    const SpBinGeom g = sp_bin_geometry(N);
    if (cshift) *cshift = g.cshift;
    if (nch) *nch = g.nch;
    if (nbins) *nbins = g.nbins;
    if (binned_ok) *binned_ok = g.ok ? 1 : 0;
    return D2G_OK;
}

// diagnostics: the pair list and the sorted order of the last prepare, copied to the host (synchronises `s`)
int d2g_bitslice_debug_read(d2g_ctx *ctx, const d2g_cmp_set *set, hipStream_t s, uint64_t *pairs_out, size_t cap, size_t *npairs, uint32_t *root_out /* [N] or null */) {
    *npairs = 0;
    if (!set->srt_valid || !set->sp) { D2G_HIP(ctx, hipStreamSynchronize(s)); return D2G_OK; }
    const SpState &sp = *set->sp;
    uint32_t n = 0;
    D2G_HIP(ctx, hipMemcpyAsync(&n, sp.d_plctl, 4, hipMemcpyDeviceToHost, s));
    D2G_HIP(ctx, hipStreamSynchronize(s));
    const size_t m = std::min<size_t>(std::min<size_t>(n, sp.plist_cap), cap);
    if (m && pairs_out) D2G_HIP(ctx, hipMemcpy(pairs_out, sp.d_plist, m * 8, hipMemcpyDeviceToHost));
    if (root_out) D2G_HIP(ctx, hipMemcpy(root_out, sp.d_label + set->Npad, set->N * 4, hipMemcpyDeviceToHost));
    *npairs = m;
    return D2G_OK;
}

// what the engines of one multi-GPU job must agree on: the RESOLVED values (a rank with D2G_SP_LINK=1 and one that leaves it unset resolve the
// same kernels -- ADVICE r5: the textual form refused them as different)
uint64_t d2g_k2_tuning_hash(const d2g_ctx *ctx) {
    const d2g_k2_tuning &t = ctx->k2;
    const long long v[] = {t.sparse, (long long)t.min_n, t.link, (long long)(t.tile_frac * 1e6), t.olink, t.emit_big, t.ride, t.remember, (long long)t.list_div, (long long)t.long_list,
                           t.list_form, t.predict, t.sort ? 1 : 0, t.tagbits_max, t.nsplit_req, t.merge, t.rank_share};
    uint64_t h = 1469598103934665603ull;
    for (long long x : v) for (int b = 0; b < 8; ++b) { h ^= (uint64_t)(x >> (8 * b)) & 0xFF; h *= 1099511628211ull; }
    return h;
}

std::string d2g_k2_tuning_json(const d2g_ctx *ctx) {
    const d2g_k2_tuning &t = ctx->k2;
    char b[640];
    std::snprintf(b, sizeof b, "{\"D2G_BS_SPARSE\": %d, \"D2G_BS_SPARSE_MIN_N\": %zu, \"D2G_BS_SORT\": %d, \"D2G_SP_LINK\": %d, \"D2G_SP_OLINK\": %d, \"D2G_SP_TILE_FRAC\": %.3f, "
                  "\"D2G_SP_LIST_DIV\": %zu, \"D2G_SP_LONG_LIST\": %zu, \"D2G_SP_LIST_FORM\": %d, \"D2G_SP_PREDICT\": %d, \"D2G_SP_REMEMBER\": %d, \"D2G_SP_RIDE\": %d, \"D2G_SP_EMIT_BIG\": %d, \"D2G_K2_MERGE\": %d, \"D2G_BS_ID16\": %d, \"D2G_SP_RANK_SHARE\": %d}",
                  t.sparse ? 1 : 0, t.min_n, t.sort ? 1 : 0, t.link, t.olink, t.tile_frac, t.list_div, t.long_list, t.list_form, t.predict, t.remember, t.ride, t.emit_big, t.merge, t.id16, t.rank_share);
    return b;
}

void d2g_warm_k2_bitslice() { hipFuncAttributes a; (void)hipFuncGetAttributes(&a, reinterpret_cast<const void *>(&bs_colplan_kernel)); }

#ifdef D2G_RANK_TRACE
extern "C" int d2g_debug_rank_trace(unsigned long long *out, size_t n) {
    return hipMemcpyFromSymbol(out, HIP_SYMBOL(g_rank_trace), std::min<size_t>(n, 8192 * 16) * 8) == hipSuccess ? 0 : -1;
}
#endif
#ifdef D2G_SP_TRACE
// variant builds only: the time stamps of the last sparse pair kernel (tools/sp_trace.py)
extern "C" int d2g_debug_emit_trace(unsigned long long *out, size_t n) {
    return hipMemcpyFromSymbol(out, HIP_SYMBOL(g_emit_trace), std::min<size_t>(n, 4096 * 16) * 8) == hipSuccess ? 0 : -1;
}
extern "C" int d2g_debug_sp_trace(unsigned long long *out, size_t n) {
    return hipMemcpyFromSymbol(out, HIP_SYMBOL(g_sp_trace), std::min<size_t>(n, 16384 * 8) * 8) == hipSuccess ? 0 : -1;
}
#endif
