// edit_selftest.cpp -- the host side of edit distances (K2h; the reader in d2g_seqpack.cpp, the checks in d2g_host.cpp) under ASan + UBSan, no GPU:
//   1. d2g_seqrecs against the seqpack reader (d2g_seqpack_add_fastx_by_record): the same number of records and the same names on FASTA,
//      FASTQ, CRLF line ends, a last record without a line feed, an empty record, a FASTQ record that the walk drops; the bytes kept are
//      the sequence lines as they stand (case, N, anything), qualities ignored; the path form on a file
//   2. d2g_seqset_check: what it accepts, its refusals and their words
//   3. d2g_seqset_recode_map: sigma and the order of the codes
#include "../../../include/d2g.h"
#include <cstdio>
#include <cstring>
#include <string>
#include <unistd.h>
#include <vector>

#define REQUIRE(c) do { if (!(c)) { std::fprintf(stderr, "edit selftest failed: %s (line %d)\n", #c, __LINE__); return 1; } } while (0)

struct Recs { std::vector<std::string> names, seqs; };

static int read_both(const std::string &buf, Recs &out) {
    d2g_seqrecs *sr = nullptr;
    d2g_seqpack *sp = nullptr;
    REQUIRE(d2g_seqrecs_create(&sr) == D2G_OK && d2g_seqpack_create(4, &sp) == D2G_OK);
    // exact-size heap copies: ASan sees any read past the input
    std::vector<char> a(buf.begin(), buf.end()), b(buf.begin(), buf.end());
    REQUIRE(d2g_seqrecs_add_fastx(sr, a.data(), a.size()) == D2G_OK);
    REQUIRE(d2g_seqpack_add_fastx_by_record(sp, b.data(), b.size()) == D2G_OK);
    const size_t n = d2g_seqrecs_nrecords(sr);
    REQUIRE(n == d2g_seqpack_ngenomes(sp));
    const uint64_t *off = d2g_seqrecs_off(sr);
    const uint8_t *bytes = d2g_seqrecs_bytes(sr);
    REQUIRE(off[0] == 0);
    out.names.clear(); out.seqs.clear();
    for (size_t i = 0; i < n; ++i) {
        REQUIRE(std::strcmp(d2g_seqrecs_name(sr, i), d2g_seqpack_name(sp, i)) == 0);
        REQUIRE(off[i + 1] >= off[i]);
        out.names.emplace_back(d2g_seqrecs_name(sr, i));
        out.seqs.emplace_back(reinterpret_cast<const char *>(bytes) + off[i], off[i + 1] - off[i]);
    }
    REQUIRE(d2g_seqset_check(bytes, off, n, off[n], nullptr, 0) == D2G_OK);
    REQUIRE(std::strcmp(d2g_seqrecs_name(sr, n), "") == 0);
    d2g_seqrecs_destroy(sr);
    d2g_seqpack_destroy(sp);
    return 0;
}

static int reader() {
    Recs r;
    // FASTA: several lines per record, lower case, N, a description after the name
    REQUIRE(read_both(">r1 first record\nACGTNN\nacgt\n>r2\nTTTT\n", r) == 0);
    REQUIRE(r.names == (std::vector<std::string>{"r1", "r2"}) && r.seqs == (std::vector<std::string>{"ACGTNNacgt", "TTTT"}));
    // FASTQ: qualities ignored, also one that begins with '@' or '>'
    REQUIRE(read_both("@q1\nACGT\n+\n@>II\n@q2 x\nGGN\n+q2\nIII\n", r) == 0);
    REQUIRE(r.names == (std::vector<std::string>{"q1", "q2"}) && r.seqs == (std::vector<std::string>{"ACGT", "GGN"}));
    // CRLF
    REQUIRE(read_both(">c1\r\nACGT\r\nAC\r\n>c2\r\nG\r\n", r) == 0);
    REQUIRE(r.names == (std::vector<std::string>{"c1", "c2"}) && r.seqs[0] == "ACGTAC");
    // a last record without a line feed
    REQUIRE(read_both(">a\nAC\n>b\nGGTT", r) == 0);
    REQUIRE(r.names == (std::vector<std::string>{"a", "b"}) && r.seqs == (std::vector<std::string>{"AC", "GGTT"}));
    // an empty record is kept, with length 0 -- in the middle and at the end
    REQUIRE(read_both(">a\nAC\n>empty\n>b\nG\n>last\n", r) == 0);
    REQUIRE(r.names == (std::vector<std::string>{"a", "empty", "b", "last"}) && r.seqs == (std::vector<std::string>{"AC", "", "G", ""}));
    // a FASTQ record whose quality length differs is dropped and ends the input, for both readers alike
    REQUIRE(read_both("@ok\nACGT\n+\nIIII\n@bad\nACGT\n+\nII\n@never\nAC\n+\nII\n", r) == 0);
    REQUIRE(r.names.size() >= 1 && r.names[0] == "ok" && r.seqs[0] == "ACGT");
    for (const auto &s : r.seqs) REQUIRE(s.find('I') == std::string::npos);
    // bytes are bytes: protein letters, digits, high bytes
    REQUIRE(read_both(">p\nMKV*\x80\xff" "09\n", r) == 0);
    REQUIRE(r.seqs[0] == std::string("MKV*\x80\xff" "09"));
    // a long line (the packer's block path must not run for raw records)
    const std::string longseq(1000, 'G');
    REQUIRE(read_both(">l\n" + longseq + "\n>m\nAC\n", r) == 0);
    REQUIRE(r.seqs[0] == longseq && r.seqs[1] == "AC");
    REQUIRE(read_both("", r) == 0 && r.names.empty());
    // the path form
    char path[] = "/tmp/d2g_edit_selftest_XXXXXX";
    const int fd = mkstemp(path);
    REQUIRE(fd >= 0);
    const std::string fa = ">x\nACGT\n>y\nAAA\nCC\n";
    REQUIRE(write(fd, fa.data(), fa.size()) == (ssize_t)fa.size());
    close(fd);
    d2g_seqrecs *sr = nullptr;
    REQUIRE(d2g_seqrecs_create(&sr) == D2G_OK);
    REQUIRE(d2g_seqrecs_add_path(sr, path) == D2G_OK);
    unlink(path);
    REQUIRE(d2g_seqrecs_nrecords(sr) == 2 && d2g_seqrecs_off(sr)[2] == 9 && std::memcmp(d2g_seqrecs_bytes(sr), "ACGTAAACC", 9) == 0);
    REQUIRE(std::strcmp(d2g_seqrecs_name(sr, 1), "y") == 0);
    REQUIRE(d2g_seqrecs_add_path(sr, "/nonexistent/d2g_edit_selftest") == D2G_ERR_IO);
    d2g_seqrecs_destroy(sr);
    REQUIRE(d2g_seqrecs_add_path(nullptr, path) == D2G_ERR_INVALID && d2g_seqrecs_nrecords(nullptr) == 0);
    return 0;
}

static int check() {
    char msg[256] = "";
    const std::vector<uint8_t> bytes(10, 'A');
    const uint64_t off[] = {0, 3, 3, 10}, not0[] = {1, 3, 10}, back[] = {0, 5, 3, 10}, shortoff[] = {0, 3, 9};
    REQUIRE(d2g_seqset_check(bytes.data(), off, 3, 10, msg, sizeof msg) == D2G_OK);
    const uint64_t zero = 0;
    REQUIRE(d2g_seqset_check(nullptr, &zero, 0, 0, nullptr, 0) == D2G_OK);
    REQUIRE(d2g_seqset_check(bytes.data(), nullptr, 3, 10, msg, sizeof msg) == D2G_ERR_INVALID && std::strstr(msg, "null off"));
    REQUIRE(d2g_seqset_check(nullptr, off, 3, 10, msg, sizeof msg) == D2G_ERR_INVALID && std::strstr(msg, "null bytes"));
    REQUIRE(d2g_seqset_check(bytes.data(), not0, 2, 10, msg, sizeof msg) == D2G_ERR_INVALID && std::strstr(msg, "begin at 0"));
    REQUIRE(d2g_seqset_check(bytes.data(), back, 3, 10, msg, sizeof msg) == D2G_ERR_INVALID && std::strstr(msg, "decreases at record 1"));
    REQUIRE(d2g_seqset_check(bytes.data(), shortoff, 2, 10, msg, sizeof msg) == D2G_ERR_INVALID && std::strstr(msg, "ends at 9") && std::strstr(msg, "10 bytes"));
    REQUIRE(d2g_seqset_check(bytes.data(), back, 3, 10, nullptr, 0) == D2G_ERR_INVALID);
    const std::vector<uint8_t> big(D2G_EDIT_MAX_LEN + 1 + 2, 'C');
    const uint64_t at_cap[] = {0, 2, 2 + D2G_EDIT_MAX_LEN}, above[] = {0, 2, 2 + D2G_EDIT_MAX_LEN + 1};
    REQUIRE(d2g_seqset_check(big.data(), at_cap, 2, 2 + D2G_EDIT_MAX_LEN, msg, sizeof msg) == D2G_OK);
    REQUIRE(d2g_seqset_check(big.data(), above, 2, big.size(), msg, sizeof msg) == D2G_ERR_UNSUPPORTED && std::strstr(msg, "record 1") && std::strstr(msg, "65536"));
    return 0;
}

static int recode() {
    uint8_t map[256];
    const std::string s = "TACGTacgNN";
    REQUIRE(d2g_seqset_recode_map(reinterpret_cast<const uint8_t *>(s.data()), s.size(), map) == 8);
    // in order of byte value: A C G N T a c g
    const char *order = "ACGNTacg";
    for (int i = 0; order[i]; ++i) REQUIRE(map[(unsigned char)order[i]] == i);
    REQUIRE(map['t'] == 0 && map[0] == 0 && map[255] == 0);                            // a value that does not occur
    REQUIRE(d2g_seqset_recode_map(nullptr, 0, map) == 1);                               // no byte at all: sigma = 1
    REQUIRE(d2g_seqset_recode_map(reinterpret_cast<const uint8_t *>("aaaa"), 4, map) == 1 && map['a'] == 0);
    std::vector<uint8_t> all(256);
    for (int i = 0; i < 256; ++i) all[i] = uint8_t(255 - i);
    REQUIRE(d2g_seqset_recode_map(all.data(), all.size(), map) == 256);
    for (int i = 0; i < 256; ++i) REQUIRE(map[i] == i);
    const uint8_t ends[] = {255, 0, 255};
    REQUIRE(d2g_seqset_recode_map(ends, 3, map) == 2 && map[0] == 0 && map[255] == 1);
    return 0;
}

int main() {
    if (reader() || check() || recode()) return 1;
    std::printf("edit selftest OK\n");
    return 0;
}
