// contain_selftest.cpp -- the host code of `dashing2 contain` under ASan + UBSan (`make sanitize`), no GPU: the database loader and both
// writers (host/contain_files.h) and the epilogue (d2g_epilogue_contain).  With a path as its argument it also checks the text of
// every entry of tests/golden/contain_fmt.txt (fmt 12.1.0's own "{:0.6g}" and "{}").
#include "../../host/contain_files.h"
#include "../../../include/d2g.h"
#include <cstdlib>
#include <cstring>
#include <unistd.h>

#define REQUIRE(c) do { if (!(c)) { std::fprintf(stderr, "contain selftest FAILED at %s:%d: %s\n", __FILE__, __LINE__, #c); return 1; } } while (0)

static bool put(const std::string &path, const void *p, size_t n) {
    std::FILE *fp = std::fopen(path.c_str(), "wb");
    if (!fp) return false;
    const bool ok = std::fwrite(p, 1, n, fp) == n;
    std::fclose(fp);
    return ok;
}
static std::string slurp_file(const std::string &path) {
    std::string s;
    if (std::FILE *fp = std::fopen(path.c_str(), "rb")) { char b[4096]; for (size_t n; (n = std::fread(b, 1, sizeof b, fp)) > 0;) s.append(b, n); std::fclose(fp); }
    return s;
}

int main(int argc, char **argv) {
    using namespace d2h;
    char tmpl[] = "/tmp/d2g_contain_selftest_XXXXXX";
    REQUIRE(mkdtemp(tmpl) != nullptr);
    const std::string dir = tmpl;
    // ---- the loader: header fields, rows, names
    const uint32_t S = 3, k = 21;
    std::vector<unsigned char> file(24 + 2 * S * 8);
    const uint32_t hdr[4] = {0u | (1u << 8), S, k, k};
    const uint64_t seed = 7, keys[6] = {1, 2, ~0ull, 4, 5, ~0ull};
    std::memcpy(file.data(), hdr, 16); std::memcpy(file.data() + 16, &seed, 8); std::memcpy(file.data() + 24, keys, sizeof keys);
    const std::string dbp = dir + "/db.kmer64";
    REQUIRE(put(dbp, file.data(), file.size()));
    ContainDb db;
    std::string err;
    REQUIRE(load_contain_db(dbp, db, err));                       // no names file: 0 .. nrefs-1, where the reference throws
    REQUIRE(db.dtype == 0 && db.canon && db.S == S && db.k == k && db.w == k && db.seed == 7 && db.nrefs == 2);
    REQUIRE(db.keys.size() == 6 && std::memcmp(db.keys.data(), keys, sizeof keys) == 0);
    REQUIRE(db.names.size() == 2 && db.names[0] == "0" && db.names[1] == "1");
    REQUIRE(put(dbp + ".names.txt", "a b.fa\nc.fa\n", 12));
    REQUIRE(load_contain_db(dbp, db, err) && db.names.size() == 2 && db.names[0] == "a b.fa" && db.names[1] == "c.fa");
    REQUIRE(put(dbp + ".names.txt", "a.fa\n", 5));
    REQUIRE(!load_contain_db(dbp, db, err) && err == "Database corrupted; wrong number of names.");
    REQUIRE(put(dbp + ".names.txt", "a.fa\nb.fa\n\n", 11));     // an empty line is a name, as std::getline gives it
    REQUIRE(!load_contain_db(dbp, db, err) && err == "Database corrupted; wrong number of names.");
    // a payload that is a multiple of S bytes but not of whole rows: what the reference's `% S` lets through
    const std::string bad = dir + "/bad.kmer64";
    REQUIRE(put(bad, file.data(), 24 + S * 8 + S));
    REQUIRE(!load_contain_db(bad, db, err) && err == "Database corrupted (not a multiple of uint64_t size). Regenerate?");
    REQUIRE(put(bad, file.data(), 24 + S * 8 + 8));
    REQUIRE(!load_contain_db(bad, db, err) && err.find("Database corrupted (not a multiple") == 0);
    REQUIRE(put(bad, file.data(), 23));
    REQUIRE(!load_contain_db(bad, db, err) && err.find("24-byte header") != std::string::npos);
    REQUIRE(!load_contain_db(dir + "/none.kmer64", db, err) && err.find("none.kmer64") != std::string::npos);
    REQUIRE(put(bad, file.data(), 24));                          // no references at all is a database
    REQUIRE(load_contain_db(bad, db, err) && db.nrefs == 0 && db.names.empty() && db.keys.empty());
    { uint32_t h0[4] = {2u, 0u, k, k}; std::memcpy(file.data(), h0, 16); REQUIRE(put(bad, file.data(), 24 + 8)); }
    REQUIRE(load_contain_db(bad, db, err) && db.S == 0 && db.dtype == 2 && !db.canon);     // S = 0 is the caller's refusal, not a division here

    // ---- the epilogue: coverage in double then float, depth the integer quotient, 0 where nothing matched
    const uint32_t m[5] = {0, 1, 3, 1024, 7}, ms[5] = {5, 9, 10, 4294967295u, 6};      // 4294967295 = a sum that wrapped to just below 2^32
    float cov[5], dep[5];
    REQUIRE(d2g_epilogue_contain(m, ms, 5, 1024, cov, dep) == D2G_OK);
    REQUIRE(cov[0] == 0.f && dep[0] == 0.f);
    REQUIRE(cov[1] == float((1. / 1024) * 1) && dep[1] == 9.f);
    REQUIRE(cov[2] == float((1. / 1024) * 3) && dep[2] == 3.f);                         // 10 / 3 = 3, not 3.33
    REQUIRE(cov[3] == 1.f && dep[3] == float(4294967295u / 1024u));
    REQUIRE(dep[4] == 0.f && cov[4] == float((1. / 1024) * 7));                         // 6 / 7 = 0
    REQUIRE(d2g_epilogue_contain(m, ms, 5, 10, cov, dep) == D2G_OK && cov[2] == float((1. / 10) * 3));
    REQUIRE(d2g_epilogue_contain(m, ms, 5, 0, cov, dep) == D2G_ERR_INVALID);
    REQUIRE(d2g_epilogue_contain(nullptr, nullptr, 0, 4, nullptr, nullptr) == D2G_OK);

    // ---- the writers
    const std::vector<std::string> names = {"r0.fa", "r 1.fa"}, queries = {"q.fq", "dir/q2.fa.gz"};
    const float c2[4] = {0.f, float((1. / 1024) * 3), 1.f, float((1. / 10) * 3)}, d2[4] = {0.f, 3.f, 12.f, 1.f};
    const std::string tp = dir + "/out.txt", bp = dir + "/out.bin";
    std::FILE *fp = std::fopen(tp.c_str(), "wb");
    REQUIRE(fp && write_contain_text(fp, names, queries, c2, d2));
    std::fclose(fp);
    REQUIRE(slurp_file(tp) == "#Dashing2 contain - a list of coverage %%s for the set of references, + mean coverage levels.\n"
                              "#Each matrix entry consists of <coverage%%:mean depth of coverage>\n"
                              "##References:\tr0.fa\tr 1.fa\n"
                              "q.fq\t0%:0\t0.292969%:3\n"
                              "dir/q2.fa.gz\t100%:12\t30%:1\n");
    fp = std::fopen(bp.c_str(), "wb");
    REQUIRE(fp && write_contain_binary(fp, 2, 2, c2, d2));
    std::fclose(fp);
    const std::string b = slurp_file(bp);
    const uint64_t bh[2] = {2, 2};
    REQUIRE(b.size() == 16 + 32 && std::memcmp(b.data(), bh, 16) == 0 && std::memcmp(b.data() + 16, c2, 16) == 0 && std::memcmp(b.data() + 32, d2, 16) == 0);
    fp = std::fopen(tp.c_str(), "wb");                            // no references, no queries' entries: the header and bare paths
    REQUIRE(fp && write_contain_text(fp, {}, queries, nullptr, nullptr));
    std::fclose(fp);
    REQUIRE(slurp_file(tp).find("##References:\nq.fq\ndir/q2.fa.gz\n") != std::string::npos);

    // ---- the golden: "g <S> <m> <text>" = {:0.6g} of 100.f * (float)((1.0 / S) * m), "i <v> <text>" = {} of (float)v
    size_t checked = 0;
    if (argc > 1) {
        std::FILE *gf = std::fopen(argv[1], "r");
        REQUIRE(gf != nullptr);
        char kind; unsigned long long a, bb; char text[64];
        while (std::fscanf(gf, " %c %llu %llu %63s", &kind, &a, &bb, text) == 4) {
            char out[64];
            size_t n = 0;
            if (kind == 'g') n = format_g6(100.f * float((1. / double(a)) * double(bb)), out);
            else if (kind == 'i') n = format_float(float(bb), out);
            else REQUIRE(!"golden line of an unknown kind");
            if (std::string(out, n) != text) { std::fprintf(stderr, "contain selftest FAILED: %c %llu %llu: golden %s, got %.*s\n", kind, a, bb, text, int(n), out); return 1; }
            ++checked;
        }
        std::fclose(gf);
        REQUIRE(checked > 2000);
    }
    const std::string rm = "rm -rf '" + dir + "'";
    REQUIRE(std::system(rm.c_str()) == 0);
    std::printf("contain selftest OK (%zu golden entries)\n", checked);
    return 0;
}
