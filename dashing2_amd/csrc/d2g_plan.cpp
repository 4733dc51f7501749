// d2g_plan.cpp -- the checks of a packed run stream and the launch plan over it (d2g_plan.h): plain host arithmetic.
#include "d2g_plan.h"
#include "d2g_alphabet.h"
#include "../../include/d2g.h"
#include <algorithm>
#include <cstring>

namespace {
int refuse(std::string &err, const char *msg, int status = D2G_ERR_INVALID) { err = msg; return status; }
}  // namespace

int d2g_plan_build(const PackedRuns &in, PlanHost &p, std::string &err) {
    const size_t nrun = in.nrun, n = in.n;
    const int k = in.k;
    if (!in.genome_run_off || (nrun && !(in.run_len && in.run_start))) return refuse(err, "oph plan: null table");
    if (in.alphabet != D2G_ALPHABET_DNA) {
        // K1a: what a protein alphabet refuses, before anything else is looked at
        if (!d2g_is_protein(in.alphabet)) return refuse(err, "unknown alphabet");
        if (in.canon != 0) return refuse(err, "a protein alphabet has no canonical k-mers: canon must be 0");
        if (k >= 1 && k > d2g_alphabet_max_k_of(in.alphabet))
            return refuse(err, "k exceeds the alphabet's largest exact k (20 letters: 14, 14: 16, 8: 21, 6: 24)", D2G_ERR_UNSUPPORTED);
        if (in.w > k) return refuse(err, "a window (-w > k) with a protein alphabet: the windowed walker is DNA only", D2G_ERR_UNSUPPORTED);
    }
    if (k < 1 || k > 32) return refuse(err, "k must be in [1,32] (exact 2-bit encoding path)", D2G_ERR_UNSUPPORTED);
    if (d2g_window_q(k, in.w) > D2G_WINDOW_MAX_Q)
        return refuse(err, "window too wide: -w may exceed k by at most 4095 (a window of 4096 k-mers)", D2G_ERR_UNSUPPORTED);
    if (in.genome_run_off[n] != nrun) return refuse(err, "oph plan: genome_run_off[n] != nrun");
    if (nrun >= (1ull << 32)) return refuse(err, "oph plan: too many runs");
    p.chunk_off.assign(nrun + 1, 0);
    for (size_t r = 0; r < nrun; ++r) {
        if (in.run_len[r] < (uint32_t)k) return refuse(err, "run shorter than k");
        const uint64_t nk = d2g_run_emissions_of(in.run_len[r], k, in.w);
        p.chunk_off[r + 1] = p.chunk_off[r] + (nk + K1_CHUNK - 1) / K1_CHUNK;
        p.nkmers += nk;
        p.nbases += in.run_len[r];
    }
    for (size_t g = 0; g < n; ++g) {
        const size_t r0 = in.genome_run_off[g], r1 = in.genome_run_off[g + 1];
        if (!(r1 >= r0 && r1 <= nrun)) return refuse(err, "genome_run_off not monotone");
        const uint64_t cbeg = p.chunk_off[r0], cend = p.chunk_off[r1];
        size_t r = r0;
        for (uint64_t c = cbeg; c < cend; c += K1_BLOCK_CHUNKS) {
            const uint32_t nc = (uint32_t)std::min<uint64_t>(K1_BLOCK_CHUNKS, cend - c);
            while (p.chunk_off[r + 1] <= c) ++r;
            size_t rl = r;
            while (p.chunk_off[rl + 1] < c + nc) ++rl;
            p.bg.push_back((uint32_t)g); p.bc0.push_back(c); p.bn.push_back(nc);
            p.blo.push_back((uint32_t)r); p.bhi.push_back((uint32_t)rl + 1);
        }
    }
    if (p.bg.size() >= (1ull << 31)) return refuse(err, "oph plan: too many workgroups; sketch in smaller batches");
    return D2G_OK;
}

int d2g_plan_check_tail(const PackedRuns &in, std::string &err) {
    if (!in.nrun) return D2G_OK;
    if (!in.run_start || !in.run_len) return refuse(err, "oph plan: null table");
    uint64_t maxend = 0;
    for (size_t r = 0; r < in.nrun; ++r) maxend = std::max<uint64_t>(maxend, in.run_start[r] + in.run_len[r]);
    const uint64_t stream_bytes = in.alphabet != D2G_ALPHABET_DNA ? maxend : (maxend + 3) / 4;     // a byte per residue, four bases per byte
    if (in.packed_bytes < stream_bytes + 64) return refuse(err, "packed stream lacks the 64-byte tail pad");
    return D2G_OK;
}

int d2g_plan_check_count_range(const PackedRuns &in, std::string &err) {
    if (!in.genome_run_off || (in.nrun && !in.run_len) || in.k < 1) return D2G_OK;
    for (size_t g = 0; g < in.n; ++g) {
        uint64_t nk = 0;
        for (uint64_t r = in.genome_run_off[g]; r < in.genome_run_off[g + 1] && r < in.nrun; ++r)
            nk += d2g_run_emissions_of(in.run_len[r], in.k, in.w);
        if (nk >= (1ull << 32))
            return refuse(err, "k-mer counts of a genome with 2^32 k-mers or more (the reference's uint32 counts wrap there)", D2G_ERR_UNSUPPORTED);
    }
    return D2G_OK;
}

extern "C" uint64_t d2g_run_emissions(uint64_t len, int k, int w) { return k >= 1 ? d2g_run_emissions_of(len, k, w) : 0; }

extern "C" int d2g_alphabet_size(int alphabet) { return d2g_alphabet_size_of(alphabet); }
extern "C" int d2g_alphabet_max_k(int alphabet) { return d2g_alphabet_max_k_of(alphabet); }
extern "C" int d2g_alphabet_code(int alphabet, int byte) { return byte >= 0 && byte < 256 ? d2g_alphabet_code_of(alphabet, (unsigned char)byte) : -1; }
extern "C" const char *d2g_alphabet_name(int alphabet) {
    switch (alphabet) {
    case D2G_ALPHABET_DNA: return "DNA";
    case D2G_ALPHABET_PROTEIN20: return "PROTEIN20";
    case D2G_ALPHABET_PROTEIN_3BIT: return "PROTEIN_3BIT";
    case D2G_ALPHABET_PROTEIN_14: return "PROTEIN_14";
    case D2G_ALPHABET_PROTEIN_6: return "PROTEIN_6";
    default: return "";
    }
}
extern "C" int d2g_key_bits(int k, int alphabet) { return d2g_key_bits_of(k, alphabet); }

PlanLayout d2g_plan_layout(size_t nrun, size_t nblk) {
    PlanLayout l{};
    size_t off = 0;
    auto piece = [&off](size_t bytes) { const size_t at = off; off = (off + bytes + 255) & ~size_t(255); return at; };
    l.run_start = piece(nrun * 8);
    l.run_chunk_off = piece((nrun + 1) * 8);
    l.blk_chunk0 = piece(nblk * 8);
    l.run_len = piece(nrun * 4);
    l.blk_genome = piece(nblk * 4);
    l.blk_nchunks = piece(nblk * 4);
    l.blk_run_lo = piece(nblk * 4);
    l.blk_run_hi = piece(nblk * 4);
    l.total = off;
    return l;
}

void d2g_plan_fill(uint8_t *arena, const PlanLayout &l, const PackedRuns &in, const PlanHost &p) {
    auto put = [arena](size_t at, const void *src, size_t bytes) { if (bytes) std::memcpy(arena + at, src, bytes); };
    const size_t nblk = p.bg.size();
    put(l.run_start, in.run_start, in.nrun * 8);
    put(l.run_len, in.run_len, in.nrun * 4);
    put(l.run_chunk_off, p.chunk_off.data(), p.chunk_off.size() * 8);
    put(l.blk_chunk0, p.bc0.data(), nblk * 8);
    put(l.blk_genome, p.bg.data(), nblk * 4);
    put(l.blk_nchunks, p.bn.data(), nblk * 4);
    put(l.blk_run_lo, p.blo.data(), nblk * 4);
    put(l.blk_run_hi, p.bhi.data(), nblk * 4);
}
