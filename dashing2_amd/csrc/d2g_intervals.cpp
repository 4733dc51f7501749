// d2g_intervals.cpp -- interval inputs (BED) on the host: XXH3_64bits of a chromosome name, the line parser, the launch plan of K1i and
// the sweep behind --multiset (d2g_intervals.h, include/d2g.h "K1i").  Mirrors reference src/bedsketch.cpp:36-46 line for line where
// it parses; no HIP, no context.
//
// d2g_xxh3_64 restates the short-input arms (0 .. 240 bytes, seed 0, default secret) of XXH3_64bits from the published xxHash
// specification.  The 192-byte default secret and the prime constants are those of xxHash:
//
//   xxHash - Extremely Fast Hash algorithm
//   Copyright (C) 2012-2023 Yann Collet
//   BSD 2-Clause License (https://www.opensource.org/licenses/bsd-license.php)
//
//   Redistribution and use in source and binary forms, with or without modification, are permitted provided that the following
//   conditions are met:
//     * Redistributions of source code must retain the above copyright notice, this list of conditions and the following disclaimer.
//     * Redistributions in binary form must reproduce the above copyright notice, this list of conditions and the following
//       disclaimer in the documentation and/or other materials provided with the distribution.
//   THIS SOFTWARE IS PROVIDED BY THE COPYRIGHT HOLDERS AND CONTRIBUTORS "AS IS" AND ANY EXPRESS OR IMPLIED WARRANTIES, INCLUDING, BUT
//   NOT LIMITED TO, THE IMPLIED WARRANTIES OF MERCHANTABILITY AND FITNESS FOR A PARTICULAR PURPOSE ARE DISCLAIMED. IN NO EVENT SHALL
//   THE COPYRIGHT OWNER OR CONTRIBUTORS BE LIABLE FOR ANY DIRECT, INDIRECT, INCIDENTAL, SPECIAL, EXEMPLARY, OR CONSEQUENTIAL DAMAGES
//   (INCLUDING, BUT NOT LIMITED TO, PROCUREMENT OF SUBSTITUTE GOODS OR SERVICES; LOSS OF USE, DATA, OR PROFITS; OR BUSINESS
//   INTERRUPTION) HOWEVER CAUSED AND ON ANY THEORY OF LIABILITY, WHETHER IN CONTRACT, STRICT LIABILITY, OR TORT (INCLUDING NEGLIGENCE
//   OR OTHERWISE) ARISING IN ANY WAY OUT OF THE USE OF THIS SOFTWARE, EVEN IF ADVISED OF THE POSSIBILITY OF SUCH DAMAGE.
#include "d2g_intervals.h"
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>
#include <unordered_map>

namespace {

const uint8_t XSECRET[192] = {
    0xb8, 0xfe, 0x6c, 0x39, 0x23, 0xa4, 0x4b, 0xbe, 0x7c, 0x01, 0x81, 0x2c, 0xf7, 0x21, 0xad, 0x1c,
    0xde, 0xd4, 0x6d, 0xe9, 0x83, 0x90, 0x97, 0xdb, 0x72, 0x40, 0xa4, 0xa4, 0xb7, 0xb3, 0x67, 0x1f,
    0xcb, 0x79, 0xe6, 0x4e, 0xcc, 0xc0, 0xe5, 0x78, 0x82, 0x5a, 0xd0, 0x7d, 0xcc, 0xff, 0x72, 0x21,
    0xb8, 0x08, 0x46, 0x74, 0xf7, 0x43, 0x24, 0x8e, 0xe0, 0x35, 0x90, 0xe6, 0x81, 0x3a, 0x26, 0x4c,
    0x3c, 0x28, 0x52, 0xbb, 0x91, 0xc3, 0x00, 0xcb, 0x88, 0xd0, 0x65, 0x8b, 0x1b, 0x53, 0x2e, 0xa3,
    0x71, 0x64, 0x48, 0x97, 0xa2, 0x0d, 0xf9, 0x4e, 0x38, 0x19, 0xef, 0x46, 0xa9, 0xde, 0xac, 0xd8,
    0xa8, 0xfa, 0x76, 0x3f, 0xe3, 0x9c, 0x34, 0x3f, 0xf9, 0xdc, 0xbb, 0xc7, 0xc7, 0x0b, 0x4f, 0x1d,
    0x8a, 0x51, 0xe0, 0x4b, 0xcd, 0xb4, 0x59, 0x31, 0xc8, 0x9f, 0x7e, 0xc9, 0xd9, 0x78, 0x73, 0x64,
    0xea, 0xc5, 0xac, 0x83, 0x34, 0xd3, 0xeb, 0xc3, 0xc5, 0x81, 0xa0, 0xff, 0xfa, 0x13, 0x63, 0xeb,
    0x17, 0x0d, 0xdd, 0x51, 0xb7, 0xf0, 0xda, 0x49, 0xd3, 0x16, 0x55, 0x26, 0x29, 0xd4, 0x68, 0x9e,
    0x2b, 0x16, 0xbe, 0x58, 0x7d, 0x47, 0xa1, 0xfc, 0x8f, 0xf8, 0xb8, 0xd1, 0x7a, 0xd0, 0x31, 0xce,
    0x45, 0xcb, 0x3a, 0x8f, 0x95, 0x16, 0x04, 0x28, 0xaf, 0xd7, 0xfb, 0xca, 0xbb, 0x4b, 0x40, 0x7e,
};
constexpr uint64_t P64_1 = 0x9E3779B185EBCA87ull, P64_2 = 0xC2B2AE3D27D4EB4Full, P64_3 = 0x165667B19E3779F9ull;
constexpr uint64_t PMX1 = 0x165667919E3779F9ull, PMX2 = 0x9FB21C651E98DF25ull;

// little-endian reads (the host is x86)
inline uint64_t rd64(const uint8_t *p) { uint64_t v; std::memcpy(&v, p, 8); return v; }
inline uint32_t rd32(const uint8_t *p) { uint32_t v; std::memcpy(&v, p, 4); return v; }
inline uint64_t rotl64(uint64_t x, int r) { return (x << r) | (x >> (64 - r)); }
inline uint64_t mul_fold(uint64_t a, uint64_t b) { const unsigned __int128 p = (unsigned __int128)a * b; return (uint64_t)p ^ (uint64_t)(p >> 64); }
inline uint64_t avalanche64(uint64_t h) { h ^= h >> 33; h *= P64_2; h ^= h >> 29; h *= P64_3; h ^= h >> 32; return h; }
inline uint64_t avalanche3(uint64_t h) { h ^= h >> 37; h *= PMX1; h ^= h >> 32; return h; }
inline uint64_t mix16(const uint8_t *in, const uint8_t *sec) { return mul_fold(rd64(in) ^ rd64(sec), rd64(in + 8) ^ rd64(sec + 8)); }

int refuse(std::string &err, const std::string &msg, int status = D2G_ERR_INVALID) { err = msg; return status; }
void put_err(char *err, size_t cap, const std::string &msg) { if (err && cap) std::snprintf(err, cap, "%s", msg.c_str()); }

}  // namespace

extern "C" uint64_t d2g_xxh3_64(const void *data, size_t len) {
    const uint8_t *in = static_cast<const uint8_t *>(data), *sec = XSECRET;
    if (len == 0) return avalanche64(rd64(sec + 56) ^ rd64(sec + 64));
    if (len <= 3) {
        const uint32_t c1 = in[0], c2 = in[len >> 1], c3 = in[len - 1];
        const uint32_t combined = (c1 << 16) | (c2 << 24) | c3 | ((uint32_t)len << 8);
        return avalanche64((uint64_t)combined ^ (uint64_t)(rd32(sec) ^ rd32(sec + 4)));
    }
    if (len <= 8) {
        const uint64_t in64 = (uint64_t)rd32(in + len - 4) + ((uint64_t)rd32(in) << 32);
        uint64_t h = in64 ^ (rd64(sec + 8) ^ rd64(sec + 16));
        h ^= rotl64(h, 49) ^ rotl64(h, 24);
        h *= PMX2;
        h ^= (h >> 35) + len;
        h *= PMX2;
        return h ^ (h >> 28);
    }
    if (len <= 16) {
        const uint64_t lo = rd64(in) ^ (rd64(sec + 24) ^ rd64(sec + 32)), hi = rd64(in + len - 8) ^ (rd64(sec + 40) ^ rd64(sec + 48));
        return avalanche3(len + __builtin_bswap64(lo) + hi + mul_fold(lo, hi));
    }
    if (len <= 128) {
        uint64_t acc = len * P64_1;
        if (len > 32) {
            if (len > 64) {
                if (len > 96) { acc += mix16(in + 48, sec + 96); acc += mix16(in + len - 64, sec + 112); }
                acc += mix16(in + 32, sec + 64); acc += mix16(in + len - 48, sec + 80);
            }
            acc += mix16(in + 16, sec + 32); acc += mix16(in + len - 32, sec + 48);
        }
        acc += mix16(in, sec); acc += mix16(in + len - 16, sec + 16);
        return avalanche3(acc);
    }
    if (len <= D2G_XXH3_MAX_LEN) {
        uint64_t acc = len * P64_1;
        const size_t rounds = len / 16;
        for (size_t i = 0; i < 8; ++i) acc += mix16(in + 16 * i, sec + 16 * i);
        uint64_t acc_end = mix16(in + len - 16, sec + 136 - 17);
        acc = avalanche3(acc);
        for (size_t i = 8; i < rounds; ++i) acc_end += mix16(in + 16 * i, sec + 16 * (i - 8) + 3);
        return avalanche3(acc + acc_end);
    }
    return 0;                                        // the long-input arm (stripes over the whole secret) is not restated
}

extern "C" int d2g_bed_parse(const char *buf, size_t len, int trim_chr, uint64_t *chrhash, uint64_t *start, uint64_t *stop, size_t cap,
                             size_t *nlines, char *err, size_t errcap) {
    if (nlines) *nlines = 0;
    if ((!buf && len) || !nlines || (cap && !(chrhash && start && stop))) { put_err(err, errcap, "d2g_bed_parse: null argument"); return D2G_ERR_INVALID; }
    if (len >= 2 && (unsigned char)buf[0] == 0x1f && (unsigned char)buf[1] == 0x8b) {
        put_err(err, errcap, "gzip-compressed BED input (the reference reads BED through a plain ifstream): decompress it first");
        return D2G_ERR_INVALID;
    }
    std::unordered_map<std::string, uint64_t> seen;  // one hash per distinct name
    std::string s, name;
    size_t nl = 0;
    for (size_t at = 0; at < len;) {
        const char *e = static_cast<const char *>(std::memchr(buf + at, '\n', len - at));
        const size_t end = e ? size_t(e - buf) : len;
        s.assign(buf + at, end - at);                // std::getline's line: NUL-terminated for strchr / strtoul, as in the reference
        at = end + 1;
        if (s.empty() || s.front() == '#') continue;
        char *p = s.data(), *p2;
        if ((p2 = std::strchr(p, '\t')) == nullptr) { put_err(err, errcap, "Malformed line: " + s); return D2G_ERR_INVALID; }
        if (trim_chr && ((*p == 'c' || *p == 'C') && p[1] == 'h' && p[2] == 'r')) p += 3;
        if (size_t(p2 - p) > D2G_XXH3_MAX_LEN) {
            put_err(err, errcap, "chromosome name of " + std::to_string(p2 - p) + " bytes: names longer than 240 bytes are outside this build's scope");
            return D2G_ERR_INVALID;
        }
        name.assign(p, size_t(p2 - p));
        auto it = seen.find(name);
        if (it == seen.end()) it = seen.emplace(name, d2g_xxh3_64(name.data(), name.size())).first;
        p = p2 + 1;
        const unsigned long a = std::strtoul(p, &p, 10), b = std::strtoul(p, &p, 10);
        if (nl < cap) { chrhash[nl] = it->second; start[nl] = a; stop[nl] = b; }
        ++nl;
    }
    *nlines = nl;
    return D2G_OK;
}

int d2g_interval_plan_build(const IntervalTables &in, IntervalPlanHost &p, std::string &err) {
    const size_t n = in.n, nint = in.nint;
    if (!in.file_off || (nint && !(in.chrhash && in.start && in.stop))) return refuse(err, "interval plan: null table");
    if (in.file_off[0] != 0 || in.file_off[n] != nint) return refuse(err, "interval plan: file_off[0] != 0 or file_off[n] != nint");
    for (size_t f = 0; f < n; ++f)
        if (!(in.file_off[f + 1] >= in.file_off[f] && in.file_off[f + 1] <= nint)) return refuse(err, "interval plan: file_off not monotone");
    p.chunk_off.assign(1, 0);
    p.file_positions.assign(n, 0);
    for (size_t f = 0; f < n; ++f) {
        uint64_t pos = 0;
        const size_t kept0 = p.hash.size();
        for (size_t j = in.file_off[f]; j < in.file_off[f + 1]; ++j) {
            if (in.start[j] >= in.stop[j]) continue;                      // `for (i = start; i < stop; ...)`: nothing
            const uint64_t l = in.stop[j] - in.start[j];
            if (l > D2G_INTERVAL_MAX_POSITIONS - pos) {
                char msg[200];
                std::snprintf(msg, sizeof msg, "interval plan: file %zu covers more than 2^44 positions (line %zu alone: %llu)", f,
                              j - (size_t)in.file_off[f], (unsigned long long)l);
                return refuse(err, msg, D2G_ERR_UNSUPPORTED);
            }
            pos += l;
            p.hash.push_back(in.chrhash[j]); p.start.push_back(in.start[j]); p.stop.push_back(in.stop[j]);
            p.chunk_off.push_back(p.chunk_off.back() + (l + K1_CHUNK - 1) / K1_CHUNK);
        }
        p.file_positions[f] = pos;
        p.npositions += pos;
        const size_t kept1 = p.hash.size();
        const uint64_t cbeg = p.chunk_off[kept0], cend = p.chunk_off[kept1];
        if ((cend - cbeg + K1_BLOCK_CHUNKS - 1) / K1_BLOCK_CHUNKS + p.bf.size() >= (1ull << 31))
            return refuse(err, "interval plan: too many workgroups; sketch in smaller batches", D2G_ERR_UNSUPPORTED);
        size_t r = kept0;
        for (uint64_t c = cbeg; c < cend; c += K1_BLOCK_CHUNKS) {
            const uint32_t nc = (uint32_t)std::min<uint64_t>(K1_BLOCK_CHUNKS, cend - c);
            while (p.chunk_off[r + 1] <= c) ++r;
            size_t rl = r;
            while (p.chunk_off[rl + 1] < c + nc) ++rl;
            p.bf.push_back((uint32_t)f); p.bc0.push_back(c); p.bn.push_back(nc);
            p.blo.push_back((uint32_t)r); p.bhi.push_back((uint32_t)rl + 1);
        }
    }
    if (p.hash.size() >= (1ull << 32)) return refuse(err, "interval plan: too many lines", D2G_ERR_UNSUPPORTED);
    return D2G_OK;
}

void d2g_interval_sweep(const IntervalTables &in, size_t j0, size_t j1, bool normalize, std::vector<uint64_t> &hash,
                        std::vector<uint64_t> &lo, std::vector<uint64_t> &hi, std::vector<double> &w) {
    std::vector<size_t> lines;                                           // the lines that cover something, by (hash, line)
    for (size_t j = j0; j < j1; ++j) if (in.start[j] < in.stop[j]) lines.push_back(j);
    std::stable_sort(lines.begin(), lines.end(), [&](size_t a, size_t b) { return in.chrhash[a] < in.chrhash[b]; });
    struct Ev { uint64_t x; size_t j; bool open; };
    std::vector<Ev> ev;
    std::set<size_t> active;                                             // ascending line numbers: the order of the map's `+=`
    for (size_t g0 = 0; g0 < lines.size();) {
        size_t g1 = g0;
        const uint64_t h = in.chrhash[lines[g0]];
        while (g1 < lines.size() && in.chrhash[lines[g1]] == h) ++g1;
        ev.clear();
        for (size_t t = g0; t < g1; ++t) { ev.push_back({in.start[lines[t]], lines[t], true}); ev.push_back({in.stop[lines[t]], lines[t], false}); }
        std::sort(ev.begin(), ev.end(), [](const Ev &a, const Ev &b) { return a.x < b.x; });
        active.clear();
        const size_t first = hash.size();
        uint64_t prev = 0;
        for (size_t e0 = 0; e0 < ev.size();) {
            const uint64_t x = ev[e0].x;
            if (!active.empty() && prev < x) {
                double sum = 0.;
                for (size_t j : active) sum += normalize ? 1. / (double)(in.stop[j] - in.start[j]) : 1.;
                if (hash.size() > first && hi.back() == prev && std::memcmp(&w.back(), &sum, 8) == 0) hi.back() = x;
                else { hash.push_back(h); lo.push_back(prev); hi.push_back(x); w.push_back(sum); }
            }
            for (; e0 < ev.size() && ev[e0].x == x; ++e0) { if (ev[e0].open) active.insert(ev[e0].j); else active.erase(ev[e0].j); }
            prev = x;
        }
        g0 = g1;
    }
}
