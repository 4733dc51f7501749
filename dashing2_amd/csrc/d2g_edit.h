// d2g_edit.h -- what the two edit-distance units share: the record set (d2g_edit.hip owns it) and the pair kernel's launch over a
// window of the set's order by length (d2g_edit_near.hip's full route).
#pragma once
#include "d2g_internal.h"
#include <vector>

struct d2g_seqset {
    d2g_ctx *ctx = nullptr;
    size_t N = 0;
    uint64_t nsym = 0, padded = 0;
    uint32_t sigma = 1, maxlen = 0;
    std::vector<uint32_t> len;         // host copy: which launch classes a row range has
    std::vector<uint32_t> sorted_len;  // host copy: len[order[p]], ascending (the window of columns a bound leaves)
    d2g_dev<uint8_t> codes;
    d2g_dev<uint64_t> doff;
    d2g_dev<uint32_t> dlen, order;
    size_t bytes = 0;
};

constexpr int EDIT_PAD = 16;               // a record's codes begin at a multiple of this and may be read to the next one
constexpr uint32_t EDIT_LDS_WORDS = 16384; // 64 KiB: one strip's table and, for queries of several strips, the two planes

// (d2g_edit.hip) edit_pair_kernel for rows [a0, a1) against the columns order[p0 .. p1) only: d(i, j) to out[(i - a0) * N + j]; the
// other words of `out` are not touched.  Enqueues, logs under "edit".
int d2g_edit_rect_window(d2g_ctx *ctx, const d2g_seqset *ss, uint32_t a0, uint32_t a1, uint32_t p0, uint32_t p1, uint32_t *out, hipStream_t s);
