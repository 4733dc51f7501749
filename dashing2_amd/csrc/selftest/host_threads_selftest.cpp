// host_threads_selftest.cpp -- the host-side THREADING of the CLI under ThreadSanitizer (`make tsan` in dashing2_amd/csrc;
// SURVEY 5 lists race detection among the reference's auxiliary tooling).  No GPU, no OpenMP (the OpenMP runtime is not
// instrumented and would only produce false reports).  It includes the very headers the CLI compiles and holds no copy of their loops:
//   ingest: host/ingest_pipeline.h + host/bounded_queue.h as `dashing2 sketch` runs them (sketch_cmd.cpp sketch_core): reader
//           threads -> raw staging buffers or d2g_seqpack -> ready queue -> several consumers -> finisher queue -> one finisher.
//           Fake device threads stand in for the GPU: they check the bytes or the base count of every group they get.
//   emit:   host/row_batches.h + host/slot_queue.h as every dense `dashing2 cmp` job runs them (cmp_dense.cpp): run_row_batches over
//           triangles, rectangles and panels with 1 - 3 fake lanes that fill their slots from (row, column), and a consumer that
//           checks and formats every row.
// The group planner is checked here too, against sizes written out by hand.
// Exit code 0 and no ThreadSanitizer report = pass.
#include "../../../include/d2g.h"
#include "../../host/bounded_queue.h"
#include "../../host/fmtfloat.h"
#include "../../host/ingest_pipeline.h"
#include "../../host/row_batches.h"
#include <algorithm>
#include <atomic>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iterator>
#include <map>
#include <random>
#include <string>
#include <thread>
#include <unistd.h>
#include <vector>

#define REQUIRE(c) do { if (!(c)) { std::fprintf(stderr, "threads selftest failed: %s (line %d)\n", #c, __LINE__); return 1; } } while (0)

using namespace d2h;

static std::string fasta(unsigned seed, size_t len) {
    std::mt19937_64 rng(seed);
    std::string s = ">g" + std::to_string(seed) + "\n";
    for (size_t i = 0; i < len; ++i) {
        s += "ACGTacgtN"[rng() % (seed % 3 ? 8 : 9)];
        if (i % 70 == 69) s += '\n';
    }
    return s + "\n";
}

static std::string slurp(const std::string &path) {
    std::ifstream f(path, std::ios::binary);
    return std::string(std::istreambuf_iterator<char>(f), std::istreambuf_iterator<char>());
}

// input files in a directory of their own, removed at the end
struct TempDir {
    std::string dir;
    std::vector<std::string> files;
    TempDir() { char t[] = "/tmp/d2g_threads_selftest_XXXXXX"; if (const char *d = mkdtemp(t)) dir = d; }
    std::string add(const std::string &name, const std::string &content) {
        const std::string p = dir + "/" + name;
        std::ofstream(p, std::ios::binary) << content;
        files.push_back(p);
        return p;
    }
    ~TempDir() { for (const auto &f : files) ::unlink(f.c_str()); if (!dir.empty()) ::rmdir(dir.c_str()); }
};

// bases in the packed stream of some input lines, from a single-threaded pass; -1: a file could not be opened
static long long bases_of(const std::vector<std::string> &lines, size_t b, size_t e, int k) {
    d2g_seqpack *sp = nullptr;
    if (d2g_seqpack_create(k, &sp) != D2G_OK) return -2;
    long long n = 0;
    for (size_t x = b; x < e && n >= 0; ++x) if (d2g_seqpack_add_path(sp, lines[x].c_str()) != D2G_OK) n = -1;
    if (n >= 0) n = (long long)d2g_seqpack_nbases(sp);
    d2g_seqpack_destroy(sp);
    return n;
}

struct Outcome {
    std::vector<int> stored;                             // per input line: how often the finisher stored it
    size_t raw_groups = 0, packed_groups = 0, ngroups = 0;
    int mismatches = 0;
    std::string error;
};

// One run of the real pipeline: `consumers` fake device threads, one finisher.  A slow consumer packs every group again itself.
static Outcome run_ingest(const std::vector<std::string> &lines, size_t limit, size_t readers, size_t nbufs, size_t max_ready, size_t consumers, bool slow) {
    const int k = 21;
    Outcome out;
    const GroupPlan plan = plan_groups(lines, limit);
    out.ngroups = plan.groups.size();
    std::vector<long long> want(plan.groups.size());
    for (size_t g = 0; g < plan.groups.size(); ++g) want[g] = bases_of(lines, plan.groups[g].first, plan.groups[g].second, k);
    IngestConfig cfg = ingest_config(plan, k, readers, nbufs == 0);
    cfg.readers = readers;
    cfg.nbufs = std::min(nbufs, std::max<size_t>(plan.groups.size(), 1));
    cfg.max_ready = max_ready ? max_ready : 2 * readers + 2;
    out.stored.assign(lines.size(), 0);
    std::atomic<int> mismatches{0};
    std::atomic<size_t> nraw{0}, npacked{0};
    {
        IngestPipeline pipe(lines, plan, cfg);
        if (pipe.buffers().size() != cfg.nbufs) ++mismatches;
        for (const auto &b : pipe.buffers()) if (!b.first || b.second != cfg.buf_bytes) ++mismatches;
        BoundedQueue<size_t> finq(plan.groups.size() + 1);
        std::thread finisher([&] {                       // stores by input index; the only writer of out.stored
            for (size_t g = 0; finq.pop(g);)
                for (size_t t = plan.groups[g].first; t < plan.groups[g].second; ++t) ++out.stored[t];
        });
        std::vector<std::thread> devs;
        for (size_t c = 0; c < consumers; ++c) devs.emplace_back([&] {
            for (IngestGroup r; pipe.next(r);) {
                if (r.failed()) continue;
                if (r.buf >= 0) {                        // raw group: the bytes of every file, where the offsets say
                    size_t i = 0;
                    for (size_t x = plan.groups[r.g].first; x < plan.groups[r.g].second; ++x)
                        for (const FileRef &fr : plan.files_of[x]) {
                            const std::string content = slurp(fr.path);
                            if (i >= r.foff.size() || r.flen[i] != content.size() || r.foff[i] + r.flen[i] > r.raw_bytes ||
                                std::memcmp(r.raw + r.foff[i], content.data(), content.size()) != 0) ++mismatches;
                            ++i;
                        }
                    if (i != r.foff.size() || r.gfo.size() != plan.groups[r.g].second - plan.groups[r.g].first + 1 || r.gfo.back() != i) ++mismatches;
                    ++nraw;
                    pipe.release_buffer(r);
                } else {
                    if ((long long)d2g_seqpack_nbases(r.sp) != want[r.g]) ++mismatches;
                    ++npacked;
                }
                if (slow && bases_of(lines, plan.groups[r.g].first, plan.groups[r.g].second, k) != want[r.g]) ++mismatches;
                finq.push(r.g);
                pipe.release(r);
            }
        });
        for (auto &th : devs) th.join();
        finq.close();
        finisher.join();
        pipe.join();
        out.error = pipe.error();
        if (pipe.t_readers() < pipe.t_read_raw() + pipe.t_host_pack() - 1e-6) ++mismatches;
    }
    out.mismatches = mismatches.load();
    out.raw_groups = nraw.load(); out.packed_groups = npacked.load();
    return out;
}

static bool all_once(const Outcome &o) { for (int s : o.stored) if (s != 1) return false; return true; }
#define REQUIRE_O(o, c) do { if (!(c)) { std::fprintf(stderr, "ingest run: %zu groups (%zu raw, %zu packed), %d mismatches, every input stored once: %d, error '%s'\n", \
                                                      (o).ngroups, (o).raw_groups, (o).packed_groups, (o).mismatches, int(all_once(o)), (o).error.c_str()); REQUIRE(c); } } while (0)

static int planner_checks() {
    const std::map<std::string, size_t> sizes = {{"a", 100}, {"b", 16}, {"c", 1}, {"d", 0}, {"big", 1000}, {"e", 32}};
    auto size_of = [&](const std::string &p) { return sizes.at(p); };
    using G = std::vector<std::pair<size_t, size_t>>;
    // rounded to 16: a 112, b 16, c 16, d 0, big 1008, e 32
    GroupPlan p = plan_groups({"a", "b", "c", "d", "big", "e"}, 144, size_of);
    REQUIRE((p.groups == G{{0, 4}, {4, 5}, {5, 6}}));                  // 112 + 16 + 16 = 144 lands exactly on the limit; big alone exceeds it
    REQUIRE((p.group_bytes == std::vector<size_t>{144, 1008, 32}));
    p = plan_groups({"a", "b", "c", "d", "big", "e"}, 143, size_of);
    REQUIRE((p.groups == G{{0, 2}, {2, 4}, {4, 5}, {5, 6}}));
    REQUIRE((p.group_bytes == std::vector<size_t>{128, 16, 1008, 32}));
    p = plan_groups({"big", "big"}, 1, size_of);                       // never an empty group
    REQUIRE((p.groups == G{{0, 1}, {1, 2}}));
    p = plan_groups({"a b", " c  d ", "e"}, 1000, size_of);            // a line is split on spaces
    REQUIRE((p.groups == G{{0, 3}}) && p.group_bytes[0] == 112 + 16 + 16 + 0 + 32);
    REQUIRE(p.files_of[0].size() == 2 && p.files_of[0][1].path == "b" && p.files_of[0][1].size == 16 && p.files_of[1].size() == 2 && p.files_of[1][0].path == "c");
    p = plan_groups({"d", "d", "d"}, 16, size_of);                     // empty files take no room
    REQUIRE((p.groups == G{{0, 3}}) && p.group_bytes[0] == 0);
    p = plan_groups({}, 16, size_of);
    REQUIRE(p.groups.empty() && p.group_bytes.empty() && p.files_of.empty());
    const IngestConfig c = ingest_config(plan_groups({"a", "b", "c", "d", "big", "e"}, 144, size_of), 21, 16, false);
    REQUIRE(c.readers == 3 && c.max_ready == 8 && c.buf_bytes == 4096 + 4096 && c.nbufs == 3);
    REQUIRE(ingest_config(plan_groups({}, 16, size_of), 21, 16, false).readers == 1);
    return 0;
}

static int ingest_checks() {
    TempDir td;
    REQUIRE(!td.dir.empty());
    std::vector<std::string> fa;
    for (int j = 0; j < 64; ++j) fa.push_back(td.add("g" + std::to_string(j) + ".fa", fasta(100 + j, 20000 + 977 * (j % 7))));
    // host parser only: no staging buffers
    Outcome o = run_ingest(fa, 1000, 6, 0, 0, 4, false);
    REQUIRE_O(o, o.ngroups == 64 && o.mismatches == 0 && o.error.empty() && all_once(o) && o.raw_groups == 0 && o.packed_groups == 64);
    // hybrid: FASTA goes to a staging buffer when one is free; FASTQ, a line of two files (one of them empty) and whatever finds no buffer are packed
    std::string fq;
    for (int i = 0; i < 60; ++i) fq += "@r" + std::to_string(i) + "\n" + fasta(900 + i, 150).substr(6, 70) + "\n+\n" + std::string(70, 'I') + "\n";
    const std::string fqp = td.add("reads.fq", fq), empty = td.add("empty.fa", "");
    std::vector<std::string> mix(fa.begin(), fa.begin() + 24);
    mix.insert(mix.begin() + 5, fqp);
    mix.insert(mix.begin() + 9, empty);
    mix.insert(mix.begin() + 13, fa[30] + " " + fa[31]);
    mix.insert(mix.begin() + 17, empty + " " + fa[32]);
    mix.push_back(fqp);
    o = run_ingest(mix, 1000, 6, 3, 0, 4, false);       // one input line per group, but the empty file takes no room: the line after it joins its group
    REQUIRE_O(o, o.ngroups == mix.size() - 1 && o.mismatches == 0 && o.error.empty() && all_once(o));
    REQUIRE_O(o, o.raw_groups >= 1 && o.packed_groups >= 2 && o.raw_groups + o.packed_groups == o.ngroups);
    // several inputs per group, raw and packed
    o = run_ingest(mix, 70000, 3, 2, 0, 2, false);
    REQUIRE_O(o, o.ngroups > 1 && o.ngroups < mix.size() && o.mismatches == 0 && o.error.empty() && all_once(o));
    // back-pressure: a ready bound of 2, one slow consumer
    o = run_ingest(fa, 1000, 6, 2, 2, 1, true);
    REQUIRE_O(o, o.ngroups == 64 && o.mismatches == 0 && o.error.empty() && all_once(o));
    // error: one missing path in the middle of 40 inputs, a limit of one input per group -- every thread joins, the error names the
    // path, everything outside the failed group is delivered.  (A path that cannot be stat()ed counts 0 bytes, so by the planner's
    // rules it opens a group that the input after it joins: that input fails with it, the other 38 arrive.)
    const std::string missing = td.dir + "/missing.fa";
    for (size_t nbufs : {size_t(0), size_t(3)}) {
        std::vector<std::string> bad(fa.begin(), fa.begin() + 39);
        bad.insert(bad.begin() + 20, missing);
        o = run_ingest(bad, 1000, 6, nbufs, 0, 4, false);
        REQUIRE_O(o, o.ngroups == 39 && o.mismatches == 0 && o.error == "Failed to open " + missing && o.raw_groups + o.packed_groups == 38);
        for (size_t t = 0; t < bad.size(); ++t)
            if (o.stored[t] != (t == 20 || t == 21 ? 0 : 1)) { std::fprintf(stderr, "input %zu stored %d time(s)\n", t, o.stored[t]); REQUIRE(false); }
    }
    // edges: one group; an empty to-do list ends at once
    o = run_ingest(mix, size_t(1) << 30, 6, 3, 0, 4, false);
    REQUIRE_O(o, o.ngroups == 1 && o.mismatches == 0 && o.error.empty() && all_once(o) && o.packed_groups == 1);
    o = run_ingest({}, 1000, 1, 0, 0, 4, false);
    REQUIRE_O(o, o.ngroups == 0 && o.mismatches == 0 && o.error.empty() && o.stored.empty());
    return 0;
}

// ---------------------------------------------------------------- row batches: the loop of every dense `cmp` job
// the value a fake lane computes for (row, column); exact in float
static float cell(size_t row, size_t col) { return float((row * 131 + col * 7) % 100003) / 8.f; }

// One run of the real run_row_batches with W fake lanes.  launch notes the batch its lane was given; finish checks it, fills its slot from (row, column)
// and raises the slot's flag; the consumer checks rows, order and values, formats them, and lowers the flag.  -> values consumed
static int row_batch_run(const CmpShape &sh, int W, size_t cap, size_t &nformatted) {
    const int nslots = 2 * W + 1;
    std::vector<std::vector<float>> slots(nslots, std::vector<float>(std::max<size_t>({cap, sh.widest, 1})));
    std::vector<std::atomic<int>> full(nslots);                          // set by finish, cleared by the consumer
    for (auto &f : full) f = 0;
    std::atomic<int> errors{0}, outstanding{0}, most{0};
    struct Seen { int lane; Batch bt; };
    std::vector<Seen> finished;                                          // producer side only, like inflight
    std::vector<Batch> inflight(W, Batch{0, 0, 0});                      // what launch gave a lane; cnt == 0: nothing
    size_t next_row = 0, sum_cnt = 0;                                    // consumer side only; read after the run
    std::string text;
    const RowBatchRun run = run_row_batches(sh, cap, W, nslots,
        [&](int lane, const Batch &bt) {
            if (lane < 0 || lane >= W || inflight[lane].cnt || !bt.cnt) { ++errors; return; }   // one batch per lane; never one without values
            inflight[lane] = bt;
        },
        [&](int lane, const Batch &bt, int slot) -> const float * {
            if (slot < 0 || slot >= nslots) { ++errors; return nullptr; }
            if (bt.r1 <= bt.r0 || (bt.cnt > cap && bt.r1 - bt.r0 != 1)) ++errors;
            if (bt.cnt && (inflight[lane].r0 != bt.r0 || inflight[lane].r1 != bt.r1 || inflight[lane].cnt != bt.cnt)) ++errors;   // the batch this lane was given
            if (!bt.cnt && inflight[lane].cnt) ++errors;
            inflight[lane].cnt = 0;
            finished.push_back({lane, bt});
            if (full[slot].exchange(1) != 0) ++errors;                   // handed out while its job is unconsumed
            const int out = ++outstanding;
            if (out > most) most = out;
            float *p = slots[slot].data();
            for (size_t i = bt.r0; i < bt.r1; ++i)
                for (size_t j = 0; j < sh.nvals(i); ++j) *p++ = cell(i, sh.symmetric ? i + 1 + j : sh.c0 + j);
            if (size_t(p - slots[slot].data()) != bt.cnt) ++errors;
            return slots[slot].data();
        },
        [&](const Batch &bt, const float *data) {
            int slot = -1;
            for (int s = 0; s < nslots; ++s) if (data == slots[s].data()) slot = s;
            if (slot < 0 || bt.r0 != next_row) { ++errors; return; }      // every row once, in ascending order
            char buf[FMT_MAX_FLOAT_CHARS + 1];
            const float *p = data;
            for (size_t i = bt.r0; i < bt.r1; ++i)
                for (size_t j = 0; j < sh.nvals(i); ++j, ++p) {
                    if (*p != cell(i, sh.symmetric ? i + 1 + j : sh.c0 + j)) ++errors;
                    text.append(buf, format_float(*p, buf));
                }
            next_row = bt.r1; sum_cnt += bt.cnt;
            --outstanding;
            if (full[slot].exchange(0) != 1) ++errors;
        });
    nformatted += sum_cnt;
    REQUIRE(errors == 0);
    REQUIRE(next_row == sh.nrows && sum_cnt == sh.total_vals && run.nbatches == finished.size() && outstanding == 0 && most <= nslots);
    for (size_t b = 0; b < finished.size(); ++b)                         // consecutive batches, dealt to the lanes in turn
        REQUIRE(finished[b].bt.r0 == (b ? finished[b - 1].bt.r1 : 0) && finished[b].lane == int(b % size_t(W)));
    if (cap >= sh.total_vals && (sh.symmetric || sh.ncol)) REQUIRE(run.nbatches == (sh.nrows ? 1 : 0));   // rows without columns go `cap` at a time
    REQUIRE(run.t_dev_busy >= 0 && run.t_emit_busy >= 0 && run.t_wall >= 0 && text.size() >= sum_cnt);
    return 0;
}

static int row_batch_checks(size_t &nformatted) {
    const CmpShape tri(true, false, 7, 0), sq(false, false, 9, 0), panel(false, true, 12, 5);
    REQUIRE(tri.nrows == 7 && tri.total_vals == 21 && tri.widest == 6 && tri.nvals(0) == 6 && tri.nvals(6) == 0 && std::string(tri.name()) == "upper triangle");
    REQUIRE(sq.nrows == 9 && sq.ncol == 9 && sq.c0 == 0 && sq.total_vals == 81 && sq.nvals(3) == 9 && std::string(sq.name()) == "square");
    REQUIRE(panel.nrows == 7 && panel.c0 == 7 && panel.c1 == 12 && panel.ncol == 5 && panel.total_vals == 35 && panel.nvals(6) == 5 && std::string(panel.name()) == "panel");
    REQUIRE(tri.slot_cap(1) == 6 && tri.slot_cap(10) == 10 && tri.slot_cap(100) == 21 && CmpShape(true, false, 0, 0).slot_cap(5) == 1 && CmpShape(true, false, 1, 0).slot_cap(5) == 1);
    const Batch b = tri.batch(1, 9);                                     // rows 1 and 2 hold 5 + 4 values, row 3 would make 12
    REQUIRE(b.r0 == 1 && b.r1 == 3 && b.cnt == 9 && panel.batch(2, 12).r1 == 4 && panel.batch(2, 12).cnt == 10 && panel.batch(6, 100).r1 == 7);
    std::vector<CmpShape> shapes;
    for (size_t ns : {0, 1, 2, 7, 200}) shapes.emplace_back(true, false, ns, 0);
    for (auto rc : {std::pair<size_t, size_t>{0, 5}, {3, 0}, {7, 5}, {64, 33}}) shapes.emplace_back(false, true, rc.first + rc.second, rc.second);   // nrows x ncol, c0 = nrows
    shapes.push_back(sq);
    for (const CmpShape &sh : shapes)
        for (int W : {1, 2, 3})
            for (size_t cap : {size_t(1), sh.widest, sh.widest + 1, sh.total_vals, sh.total_vals + 1})
                if (row_batch_run(sh, W, cap, nformatted)) {
                    std::fprintf(stderr, "row batches: %s, ns %zu, %zu rows x %zu columns from %zu, W %d, cap %zu\n", sh.name(), sh.ns, sh.nrows, sh.ncol, sh.c0, W, cap);
                    return 1;
                }
    return 0;
}

int main() {
    size_t nvals = 0;
    if (planner_checks() || ingest_checks() || row_batch_checks(nvals)) return 1;
    REQUIRE(nvals > 0);
    std::printf("host threads selftest OK (planner, ingest pipeline, row batches: %zu values formatted)\n", nvals);
    return 0;
}
