// contain_files.h -- the files of `dashing2 contain` (reference src/contain_main.cpp:160-184,245-296): the loader of a k-mer
// database (<out>.kmer64 + <out>.kmer64.names.txt, as `sketch -s -o out` writes them) and the writers of both output forms.
// No GPU, no exit: errors come back as text, so that selftest/contain_selftest.cpp runs all of it under the sanitizers.
#pragma once
#include "fmtfloat.h"
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <string>
#include <sys/stat.h>
#include <vector>

namespace d2h {

struct ContainDb {
    uint32_t dtype = 0;                      // bns::InputType, low byte of the first word: 0 = DNA
    bool canon = false;                      // bit 8 of the first word
    uint32_t S = 0, k = 0, w = 0;
    uint64_t seed = 0;                       // seedseed: XORMASK = seed_mask(seed), :170-171
    size_t nrefs = 0;
    std::vector<uint64_t> keys;              // [nrefs][S] masked k-mers
    std::vector<std::string> names;          // [nrefs]
};

constexpr size_t CONTAIN_HEADER_BYTES = 24;

// 24-byte header [u32 dtype | canon << 8][u32 S][u32 k][u32 w][u64 seed], then nrefs x S u64.  Where the reference tests the payload
// `% S` (:172) this tests whole 8 S-byte rows; without a names file the references are named 0 .. nrefs-1 (the reference's own
// branch, :179-180, forgets the / 8 and then always throws: SURVEY F21, F22).  false: `err` holds the reference's message.
inline bool load_contain_db(const std::string &path, ContainDb &db, std::string &err) {
    std::FILE *fp = std::fopen(path.c_str(), "rb");
    if (!fp) { err = "Failed to open database " + path; return false; }
    struct stat st;
    if (::fstat(fileno(fp), &st) != 0 || size_t(st.st_size) < CONTAIN_HEADER_BYTES) {
        std::fclose(fp);
        err = "Database " + path + " is shorter than its 24-byte header";
        return false;
    }
    const size_t payload = size_t(st.st_size) - CONTAIN_HEADER_BYTES;
    uint32_t hdr[4];
    if (std::fread(hdr, 4, 4, fp) != 4 || std::fread(&db.seed, 8, 1, fp) != 1) { std::fclose(fp); err = "Failed to read the header of " + path; return false; }
    db.dtype = hdr[0] & 0xFF; db.canon = (hdr[0] & 0x100) != 0;
    db.S = hdr[1]; db.k = hdr[2]; db.w = hdr[3];
    if (db.S == 0) { std::fclose(fp); db.nrefs = 0; return true; }            // refused by the caller with its own reason
    if (payload % (size_t(db.S) * 8)) {
        std::fclose(fp);
        err = "Database corrupted (not a multiple of uint64_t size). Regenerate?";
        return false;
    }
    db.nrefs = payload / (size_t(db.S) * 8);
    db.keys.resize(db.nrefs * db.S);
    const bool ok = std::fread(db.keys.data(), 8, db.keys.size(), fp) == db.keys.size();
    std::fclose(fp);
    if (!ok) { err = "Failed to read the keys of " + path; return false; }
    db.names.clear();
    const std::string nf = path + ".names.txt";
    struct stat nst;
    if (::stat(nf.c_str(), &nst) == 0 && S_ISREG(nst.st_mode)) {
        std::ifstream ifs(nf);
        for (std::string line; std::getline(ifs, line);) db.names.emplace_back(line);
    } else {
        for (size_t i = 0; i < db.nrefs; ++i) db.names.push_back(std::to_string(i));
    }
    if (db.names.size() != db.nrefs) { err = "Database corrupted; wrong number of names."; return false; }
    return true;
}

// fmt's "{:0.6g}" of a float: the float widened to double under printf's %.6g (six significant digits, trailing zeros dropped,
// exponent form below 1e-4 and from 1e6 on with at least two exponent digits) -- pinned by tests/golden/contain_fmt.txt
inline size_t format_g6(float v, char *out) { return size_t(std::snprintf(out, 32, "%.6g", double(v))); }

// "\t{:0.6g}%:{}" of 100.f * coverage and depth (the scalar arm, :291-293; the SIMD arms are not reproduced: SURVEY F23)
inline void append_contain_entry(std::string &s, float coverage, float depth) {
    char b[32 + FMT_MAX_FLOAT_CHARS];
    s += '\t';
    s.append(b, format_g6(100.f * coverage, b));
    s += "%:";
    s.append(b, format_float(depth, b));
}

// :252-257: fmt does not treat '%' specially, so both "%%" of the reference's literal reach the file
inline std::string contain_text_header(const std::vector<std::string> &names) {
    std::string s = "#Dashing2 contain - a list of coverage %%s for the set of references, + mean coverage levels.\n"
                    "#Each matrix entry consists of <coverage%%:mean depth of coverage>\n"
                    "##References:";
    for (const auto &n : names) { s += '\t'; s += n; }
    s += '\n';
    return s;
}

// the whole text output: coverage and depth are [nq][nrefs]
inline bool write_contain_text(std::FILE *fp, const std::vector<std::string> &names, const std::vector<std::string> &queries,
                               const float *coverage, const float *depth) {
    const size_t nrefs = names.size();
    std::string s = contain_text_header(names);
    for (size_t q = 0; q < queries.size(); ++q) {
        s += queries[q];
        for (size_t r = 0; r < nrefs; ++r) append_contain_entry(s, coverage[q * nrefs + r], depth[q * nrefs + r]);
        s += '\n';
        if (s.size() >= (1u << 20)) { if (std::fwrite(s.data(), 1, s.size(), fp) != s.size()) return false; s.clear(); }
    }
    return std::fwrite(s.data(), 1, s.size(), fp) == s.size();
}

// -b (:246-249): u64 nrefs, u64 nqueries, float coverage[nq][nrefs], float depth[nq][nrefs]
inline bool write_contain_binary(std::FILE *fp, size_t nrefs, size_t nq, const float *coverage, const float *depth) {
    const uint64_t hdr[2] = {uint64_t(nrefs), uint64_t(nq)};
    const size_t n = nrefs * nq;
    return std::fwrite(hdr, 8, 2, fp) == 2 && std::fwrite(coverage, 4, n, fp) == n && std::fwrite(depth, 4, n, fp) == n;
}

}  // namespace d2h
