// row_batches.h -- the shape of a dense comparison job and the ONE loop that carries its rows from the device(s) to the writer: cut the
// rows into batches, compute a batch, copy it back, finish it, hand the rows on.  Every dense `cmp` job passes it two callbacks
// (cmp_dense.cpp).  No GPU, library or OpenMP here: `make tsan` drives this very loop with fake lanes (csrc/selftest/host_threads_selftest.cpp).
#pragma once
#include "slot_queue.h"
#include <algorithm>
#include <chrono>
#include <cstddef>
#include <vector>

namespace d2h {

struct Batch { size_t r0, r1, cnt; };                          // rows [r0, r1) and the values they hold
// which rows are emitted and how many values each has (src/emitrect.cpp:211-323): the condensed upper triangle of ns sketches, the
// ns x ns square, or the panel of the first ns - nq sketches (rows) against the last nq (columns c0 .. c1)
struct CmpShape {
    bool symmetric, panel; size_t ns, nrows, c0, c1, ncol, total_vals, widest;
    CmpShape(bool sym, bool pan, size_t n, size_t nq) : symmetric(sym), panel(pan), ns(n) {
        const size_t nf = panel ? ns - nq : ns;
        c0 = panel ? nf : 0; c1 = ns; ncol = symmetric ? 0 : c1 - c0;
        nrows = symmetric ? ns : nf;
        total_vals = symmetric ? ns * (ns - 1) / 2 : nf * ncol;
        widest = symmetric ? (ns ? ns - 1 : 0) : ncol;
    }
    size_t nvals(size_t i) const { return symmetric ? ns - 1 - i : ncol; }     // values of row i
    // the batch of rows starting at r0 that fits `cap` values; a row wider than `cap` goes alone
    Batch batch(size_t r0, size_t cap) const {
        size_t r1 = r0, cnt = 0;
        if (symmetric) while (r1 < ns && (cnt == 0 || cnt + nvals(r1) <= cap)) { cnt += nvals(r1); ++r1; }
        else { r1 = std::min(nrows, r0 + std::max<size_t>(1, cap / std::max<size_t>(ncol, 1))); cnt = (r1 - r0) * ncol; }
        return {r0, r1, cnt};
    }
    // values per slot, given the size a job would like: never less than the widest row, never more than the job has
    size_t slot_cap(size_t slot_values) const { return std::max<size_t>(1, std::min(std::max(slot_values, widest), std::max<size_t>(total_vals, 1))); }
    const char *name() const { return symmetric ? "upper triangle" : panel ? "panel" : "square"; }
};

struct RowBatchRun { size_t nbatches = 0; double t_dev_busy = 0, t_emit_busy = 0, t_wall = 0; };   // busy: inside launch + finish / inside consume

// Row batches flow device -> host slot -> consumer thread (the SlotQueue): launch + finish of the next batches run while this one is
// formatted / written (the CLI ran kernel -> D2H -> emit strictly in series per batch).
//   launch(lane, batch)                  asynchronous: starts a batch that has values on lane (device) `lane`, writing its device buffers only
//   finish(lane, batch, slot) -> floats  blocks: copies the batch back and finishes it in the caller's staging of slot `slot`
//   consume(batch, floats)               on the consumer thread, in row order; the slot is free again when it returns
// The callers own the slots' memory; only indices 0 .. nslots-1 are handed out here.  2 W + 1 slots keep W lanes and the consumer busy.
// One round: up to W consecutive batches are launched back to back, one per lane, then drained in row order -- acquire a slot, finish,
// submit.  A launch therefore never waits for a free slot, and needs none: it writes device buffers only, and the finish of the batch
// that used them last has already drained them with a blocking copy.
template <class Launch, class Finish, class Consume>
RowBatchRun run_row_batches(const CmpShape &sh, size_t cap, int W, int nslots, Launch launch, Finish finish, Consume consume) {
    struct Job { Batch bt; const float *data; };
    const auto now = [] { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
    RowBatchRun run;
    const double t0 = now();
    SlotQueue<Job> q(nslots, [&consume](const Job &j) { consume(j.bt, j.data); });
    std::vector<Batch> round;
    for (size_t next = 0; next < sh.nrows;) {
        round.clear();
        double t = now();
        for (int lane = 0; lane < W && next < sh.nrows; ++lane) {
            round.push_back(sh.batch(next, cap));
            if (round.back().cnt) launch(lane, round.back());
            next = round.back().r1;
        }
        run.t_dev_busy += now() - t;
        for (size_t lane = 0; lane < round.size(); ++lane) {
            const int slot = q.acquire();
            t = now();
            const float *data = finish(int(lane), round[lane], slot);
            run.t_dev_busy += now() - t;
            q.submit(slot, Job{round[lane], data});
        }
        run.nbatches += round.size();
    }
    q.finish();
    run.t_emit_busy = q.t_busy;
    run.t_wall = now() - t0;
    return run;
}

}  // namespace d2h
