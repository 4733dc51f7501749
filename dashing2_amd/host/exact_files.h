// exact_files.h -- the files of --set / --countdict: names, writer, loader.  Plain C++ over <cstdio>, no GPU, no other file of the
// CLI: the sanitizer self-test (csrc/selftest/exact_selftest.cpp) compiles it as it is.
//   names    makedest, src/fastxmerge.cpp:70-120 + to_suffix, src/enums.cpp:28-37; count file: src/fastxsketch.cpp:314,317
//   writer   src/fastxsketch.cpp:462-489 (key file: [f64 card][u64 h x |E|]) and :507-519 (count file: [f64 c x |E|], no header)
//   loader   NOT the reference's (src/cmp_core.cpp:628-651 counts the header as a key, and both modes share one key-file name
//            while their headers differ): |E| comes from the file size minus the header, the counts and their sum from the count
//            file; the header is never read for a cardinality
#pragma once
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <string>
#include <sys/stat.h>
#include <vector>

namespace d2h {

struct ExactNameOpts { int k; bool canon; uint64_t seedseed; unsigned count_threshold; std::string outprefix; int w = 0;
                       std::string alphabet = "DNA"; };      // bns::to_string(rht_): the alphabet's name (d2g_alphabet_name), fastxmerge.cpp:117

// <path>[.seed<s>][.rc_canon].k<k>[.w<w>][.ct_threshold<c>].FullMmerSet.<DNA | PROTEIN20 | ...>.kmerset64 (.w<w> when w > k, fastxmerge.cpp:87-90) -- no .sketchsize part (fastxmerge.cpp:85), and
// FullMmerSet for BOTH modes (fastxsketch.cpp:313 passes iskmer for the count dictionary, fastxmerge.cpp:112-114)
inline std::string exact_key_file(const ExactNameOpts &o, const std::string &path) {
    std::string ret = path.substr(0, path.find_first_of(' '));
    if (!o.outprefix.empty()) {
        const auto pos = path.find_last_of('/');                 // trim_folder, src/enums.cpp:22-26, of the whole line
        ret = o.outprefix + '/' + (pos == std::string::npos ? path : path.substr(pos + 1));
    }
    if (o.seedseed != 0) ret += ".seed" + std::to_string(o.seedseed);
    if (o.canon) ret += ".rc_canon";
    ret += ".k" + std::to_string(o.k);
    if (o.w > o.k) ret += ".w" + std::to_string(o.w);
    if (o.count_threshold > 0) ret += ".ct_threshold" + std::to_string(int(o.count_threshold));
    return ret + ".FullMmerSet." + o.alphabet + ".kmerset64";
}
// the key file's name up to its last '.' plus .kmercounts.f64
inline std::string exact_count_file(const std::string &key_file) { return key_file.substr(0, key_file.find_last_of('.')) + ".kmercounts.f64"; }

inline bool exact_file_size(const std::string &path, uint64_t *size) {
    struct stat st;
    if (::stat(path.c_str(), &st) != 0 || !S_ISREG(st.st_mode)) return false;
    *size = uint64_t(st.st_size);
    return true;
}

// writes the key file with `header` (what the reference writes for the mode: |E| or the sum of the counts) and, with counts != null,
// the count file; false + err on failure
inline bool exact_write(const std::string &key_file, double header, const uint64_t *keys, const uint32_t *counts, size_t n, std::string &err) {
    std::FILE *fp = std::fopen(key_file.c_str(), "wb");
    if (!fp) { err = "Failed to open std::FILE * at" + key_file; return false; }           // fastxsketch.cpp:465
    const bool ok = std::fwrite(&header, 8, 1, fp) == 1 && (n == 0 || std::fwrite(keys, 8, n, fp) == n);
    if (std::fclose(fp) != 0 || !ok) { err = "Failed to write " + key_file; return false; }
    if (!counts) return true;
    const std::string cf = exact_count_file(key_file);
    if (!(fp = std::fopen(cf.c_str(), "wb"))) { err = "Failed to write k-mer counts"; return false; }   // :510
    std::vector<double> tmp(counts, counts + n);
    const bool okc = n == 0 || std::fwrite(tmp.data(), 8, n, fp) == n;
    if (std::fclose(fp) != 0 || !okc) { err = "Failed to write " + cf; return false; }
    return true;
}

// loads one set; want_counts: also its count file (a missing one fails with ITS path).  card = |E|, or the sum of the counts.
// Refuses: sizes that are not [8 + 8 |E|] / [8 |E|], a count that is not an integer in [1, 2^32).  Order is checked later, by
// d2g_kset_create, for all sets at once.
inline bool exact_load(const std::string &key_file, bool want_counts, std::vector<uint64_t> &keys, std::vector<uint32_t> &counts, double &card,
                       std::string &err) {
    uint64_t sz = 0;
    if (!exact_file_size(key_file, &sz)) { err = "File does not exist at " + key_file; return false; }
    if (sz < 8 || sz % 8) { err = "k-mer set file " + key_file + " has " + std::to_string(sz) + " bytes: not a header and 8-byte keys"; return false; }
    const size_t n = size_t(sz / 8 - 1);
    keys.resize(n);
    std::FILE *fp = std::fopen(key_file.c_str(), "rb");
    double header;
    const bool ok = fp && std::fread(&header, 8, 1, fp) == 1 && (n == 0 || std::fread(keys.data(), 8, n, fp) == n);
    if (fp) std::fclose(fp);
    if (!ok) { err = "Failed to read from " + key_file; return false; }
    card = double(n);
    counts.clear();
    if (!want_counts) return true;
    const std::string cf = exact_count_file(key_file);
    uint64_t csz = 0;
    if (!exact_file_size(cf, &csz)) { err = "File does not exist at " + cf; return false; }
    if (csz != uint64_t(n) * 8) { err = "k-mer count file " + cf + " has " + std::to_string(csz) + " bytes, its key file holds " + std::to_string(n) + " keys"; return false; }
    std::vector<double> tmp(n);
    fp = std::fopen(cf.c_str(), "rb");
    const bool okc = fp && (n == 0 || std::fread(tmp.data(), 8, n, fp) == n);
    if (fp) std::fclose(fp);
    if (!okc) { err = "Failed to read from " + cf; return false; }
    counts.resize(n);
    uint64_t sum = 0;
    for (size_t i = 0; i < n; ++i) {
        const double c = tmp[i];
        if (!(c >= 1. && c < 4294967296.) || c != std::floor(c)) { err = "k-mer count file " + cf + ": entry " + std::to_string(i) + " is not a count in [1, 2^32)"; return false; }
        counts[i] = uint32_t(c);
        sum += counts[i];
    }
    card = double(sum);
    return true;
}

}  // namespace d2h
