// d2g_minq.h -- the sliding-window minimum behind the windowed walker (d2g_kmers.h, -w > k): a monotone queue of at most D entries
// held in NAMED registers (every index below is a compile-time constant once the loops are unrolled: no private array, no scratch).
//
// The exact monotone queue of a window of q k-mers holds the k-mers that are smaller than everything after them: ~ln q + 0.6 entries
// on random sequence, q on a sequence of rising scores.  This one keeps the FIRST D of them (the smallest, the oldest) and forgets the
// rest: `lossy` says that entries behind the kept ones were dropped.  The front is the window's minimum as long as one kept entry is
// inside the window; when the last one leaves while `lossy` is set, the caller rolls the window's q k-mers through push() again
// (d2g_kmers.h).  Plain C++ so that the host self-test runs the same code against a brute-force minimum (selftest/window_selftest.cpp).
#pragma once
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define D2G_HD __host__ __device__ __forceinline__
#define D2G_UNROLL _Pragma("unroll")
#else
#define D2G_HD inline
#define D2G_UNROLL
#endif

// bonsai's score::Lex: a k-mer's score is the k-mer XOR this constant, compared as uint64 (a bijection: equal scores are equal k-mers)
constexpr uint64_t D2G_LEX_XOR = 0xe37e28c4271b5a2dull;

template <int D>
struct D2gMinQueue {
    uint64_t sc[D];                // scores, rising from the front
    int32_t ps[D];                 // their positions, rising too
    int32_t cnt;                   // entries held
    bool lossy;                    // entries behind sc[cnt - 1] were dropped (cnt == D when it was set; pops may have lowered cnt since)

    D2G_HD void clear() {
D2G_UNROLL
        for (int d = 0; d < D; ++d) { sc[d] = 0; ps[d] = 0; }
        cnt = 0; lossy = false;
    }
    // k-mer of score s at position t (positions rise by one per call)
    D2G_HD void push(uint64_t s, int32_t t) {
        int32_t kept = 0;                                          // entries smaller than s: a prefix, the scores rise
D2G_UNROLL
        for (int d = 0; d < D; ++d) kept += (d < cnt && sc[d] < s) ? 1 : 0;
        const bool cut = kept < cnt;                               // s ends the queue behind `kept`: whatever was dropped went with it
        const bool put = cut || (!lossy && cnt < D);
        lossy = !cut && (lossy || cnt == D);                       // nothing may follow a dropped entry: the order would have a hole
        if (put) {
D2G_UNROLL
            for (int d = 0; d < D; ++d) if (d == kept) { sc[d] = s; ps[d] = t; }
            cnt = kept + 1;
        }
    }
    // positions below `first` have left the window (at most one entry per call leaves: one k-mer leaves per step)
    D2G_HD void expire(int32_t first) {
        if (cnt > 0 && ps[0] < first) {
D2G_UNROLL
            for (int d = 0; d + 1 < D; ++d) { sc[d] = sc[d + 1]; ps[d] = ps[d + 1]; }
            --cnt;
        }
    }
    D2G_HD bool empty() const { return cnt == 0; }
    D2G_HD uint64_t front() const { return sc[0]; }
};
