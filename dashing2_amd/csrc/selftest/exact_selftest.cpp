// exact_selftest.cpp -- the host code of --set / --countdict under ASan + UBSan (`make sanitize`), no GPU: the files' names, writer and
// loader (host/exact_files.h), the validation of d2g_kset_create (d2g_kset_check) and the epilogue (d2g_epilogue_exact*).
#include "../../host/exact_files.h"
#include "../../../include/d2g.h"
#include <cstdlib>
#include <cstring>
#include <limits>
#include <unistd.h>

#define REQUIRE(c) do { if (!(c)) { std::fprintf(stderr, "exact selftest FAILED at %s:%d: %s\n", __FILE__, __LINE__, #c); return 1; } } while (0)

int main() {
    using namespace d2h;
    char tmpl[] = "/tmp/d2g_exact_selftest_XXXXXX";
    REQUIRE(mkdtemp(tmpl) != nullptr);
    const std::string dir = tmpl;
    // names
    const ExactNameOpts plain{31, true, 0, 0, ""}, full{21, false, 13, 2, "out"};
    REQUIRE(exact_key_file(plain, "d/a.fa") == "d/a.fa.rc_canon.k31.FullMmerSet.DNA.kmerset64");
    REQUIRE(exact_key_file(plain, "d/a.fa d/b.fa") == "d/a.fa.rc_canon.k31.FullMmerSet.DNA.kmerset64");
    REQUIRE(exact_key_file(full, "d/a.fa") == "out/a.fa.seed13.k21.ct_threshold2.FullMmerSet.DNA.kmerset64");
    REQUIRE(exact_count_file(exact_key_file(plain, "d/a.fa")) == "d/a.fa.rc_canon.k31.FullMmerSet.DNA.kmercounts.f64");
    // writer -> loader, both modes, and each mode picking up the other's key file
    const uint64_t keys[4] = {0, 7, 1ull << 63, ~0ull};
    const uint32_t counts[4] = {1, 4294967295u, 3, 2};
    const std::string kf = dir + "/a.kmerset64";
    std::string err;
    std::vector<uint64_t> k; std::vector<uint32_t> c; double card = -1;
    REQUIRE(exact_write(kf, 4., keys, nullptr, 4, err));
    uint64_t sz = 0;
    REQUIRE(exact_file_size(kf, &sz) && sz == 40);
    REQUIRE(exact_load(kf, false, k, c, card, err) && k.size() == 4 && c.empty() && card == 4. && std::memcmp(k.data(), keys, 32) == 0);
    REQUIRE(!exact_load(kf, true, k, c, card, err) && err.find("a.kmercounts.f64") != std::string::npos);     // the missing path is named
    REQUIRE(exact_write(kf, 4294967301., keys, counts, 4, err));                                               // the header of --countdict: the sum
    REQUIRE(exact_load(kf, true, k, c, card, err) && c.size() == 4 && c[1] == 4294967295u && card == 4294967301.);
    REQUIRE(exact_load(kf, false, k, c, card, err) && card == 4.);                                             // never the header
    REQUIRE(exact_write(dir + "/e.kmerset64", 0., nullptr, nullptr, 0, err) && exact_load(dir + "/e.kmerset64", false, k, c, card, err) && k.empty() && card == 0.);
    // refusals of the loader
    REQUIRE(!exact_load(dir + "/none.kmerset64", false, k, c, card, err) && err.find("none.kmerset64") != std::string::npos);
    { std::FILE *fp = std::fopen((dir + "/odd.kmerset64").c_str(), "wb"); REQUIRE(fp); std::fwrite("123456789012", 1, 12, fp); std::fclose(fp); }
    REQUIRE(!exact_load(dir + "/odd.kmerset64", false, k, c, card, err));
    { const double bad[4] = {1., 2.5, 3., 1.}; std::FILE *fp = std::fopen((dir + "/a.kmercounts.f64").c_str(), "wb"); REQUIRE(fp); std::fwrite(bad, 8, 4, fp); std::fclose(fp); }
    REQUIRE(!exact_load(kf, true, k, c, card, err) && err.find("entry 1") != std::string::npos);
    { const double bad[3] = {1., 2., 3.}; std::FILE *fp = std::fopen((dir + "/a.kmercounts.f64").c_str(), "wb"); REQUIRE(fp); std::fwrite(bad, 8, 3, fp); std::fclose(fp); }
    REQUIRE(!exact_load(kf, true, k, c, card, err) && err.find("24 bytes") != std::string::npos);
    // validation
    char msg[256];
    const uint64_t off[4] = {0, 2, 2, 4};
    REQUIRE(d2g_kset_check(keys, counts, off, 3, msg, sizeof msg) == D2G_OK);
    const uint64_t unsorted[4] = {0, 7, 9, 8}, dup[4] = {0, 7, 8, 8}, backoff[3] = {0, 3, 2};
    const uint32_t zero[4] = {1, 1, 0, 1};
    REQUIRE(d2g_kset_check(unsorted, nullptr, off, 3, msg, sizeof msg) == D2G_ERR_INVALID && std::strstr(msg, "not sorted") && std::strstr(msg, "set 2"));
    REQUIRE(d2g_kset_check(dup, nullptr, off, 3, msg, sizeof msg) == D2G_ERR_INVALID && std::strstr(msg, "twice"));
    REQUIRE(d2g_kset_check(keys, zero, off, 3, msg, sizeof msg) == D2G_ERR_INVALID && std::strstr(msg, "count of 0"));
    REQUIRE(d2g_kset_check(keys, nullptr, backoff, 2, msg, sizeof msg) == D2G_ERR_INVALID && std::strstr(msg, "decreases"));
    REQUIRE(d2g_kset_check(unsorted, nullptr, off, 1, msg, sizeof msg) == D2G_OK);                            // a boundary between sets is no order
    REQUIRE(d2g_kset_check(nullptr, nullptr, off, 0, nullptr, 0) == D2G_OK);
    // epilogue
    REQUIRE(d2g_epilogue_exact(30, 100., 60., D2G_SIMILARITY, 31) == float(30. / 130.));
    REQUIRE(d2g_epilogue_exact(30, 100., 60., D2G_CONTAINMENT, 31) == 0.3f && d2g_epilogue_exact(30, 100., 60., D2G_SYMMETRIC_CONTAINMENT, 31) == 0.5f);
    REQUIRE(d2g_epilogue_exact(30, 100., 60., D2G_INTERSECTION, 31) == 30.f && d2g_epilogue_exact(30, 100., 60., D2G_UNION_SIZE, 31) == 130.f);
    const float fmax = float(std::numeric_limits<long double>::max());
    const float e0 = d2g_epilogue_exact(0, 0., 0., D2G_SIMILARITY, 31), e1 = d2g_epilogue_exact(0, 5., 7., D2G_POISSON_LLR, 31);
    REQUIRE(std::memcmp(&e0, &fmax, 4) == 0 && std::memcmp(&e1, &fmax, 4) == 0);
    const uint64_t isz[6] = {1, 2, 3, 4, 5, 6};
    const double cards[4] = {10., 20., 30., 40.};
    float out[6];
    REQUIRE(d2g_epilogue_exact_ut(isz, cards, 4, 0, 4, D2G_UNION_SIZE, 31, 2, out) == D2G_OK && out[0] == 29.f && out[3] == 46.f && out[5] == 64.f);
    REQUIRE(d2g_epilogue_exact_ut(isz, cards, 4, 1, 3, D2G_UNION_SIZE, 31, 2, out) == D2G_OK && out[0] == 49.f && out[2] == 67.f);
    REQUIRE(d2g_epilogue_exact_rect(isz, cards, 4, 1, 3, 0, 3, D2G_CONTAINMENT, 31, 2, out) == D2G_OK && out[0] == float(1. / 20.) && out[5] == float(6. / 30.));
    REQUIRE(d2g_epilogue_exact_ut(isz, cards, 4, 3, 2, D2G_SIMILARITY, 31, 1, out) == D2G_ERR_INVALID);
    const std::string rm = "rm -rf '" + dir + "'";
    REQUIRE(std::system(rm.c_str()) == 0);
    std::printf("exact selftest OK\n");
    return 0;
}
