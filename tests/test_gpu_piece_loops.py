"""The host loops that cut a large call into pieces, entered on small inputs: a D2G_* switch shrinks the limit that sizes each loop
(d2g_limits.h; DESIGN.md lists them), so that its body runs more than once at the shapes of this suite.  At production size the limits
are 2^24 candidate slots, 2^30 result pairs, a third of the free device memory, 2^31 - 1 workgroups and 1024 positions per compaction
workgroup: no other test reaches a second piece.

Every test compares exact integers or bit patterns with the reference modules of the suite (knn_ref, edit_within_ref, bed_ref + the
oracle's BagMinHash, contain_ref, edit_ref, edit_dedup_ref -- none of which knows about pieces), asserts that its loop ran more than
once (the launch counts of kernel_ms where a launch per piece is logged, else the piece count computed from the resolved switch and
the shape), and runs the same input once more without the switch: bit-identical.  The unswitched run is a second check, never the
expectation."""
import ctypes

import numpy as np
import pytest

import bed_ref as B
import contain_ref as CR
import edit_dedup_cases as EC
import edit_dedup_ref as ER
import edit_ref as E
import edit_within_ref as W
import k3_seam_cases as KC
import knn_ref as KR
import oph_kmers_ref as OK
from test_gpu_bed import _ms_files
from test_gpu_edit import rect_of, seam_set, ut_of
from test_gpu_edit_dedup import dedup_of
from test_gpu_edit_within import assert_csr, near_of
from test_gpu_knn import matrix, oracle_values
from test_gpu_screen import pack

pytestmark = pytest.mark.gpu

ERR_NOMEM = -4
SWITCHES = ("D2G_KNN_CHUNK_SLOTS", "D2G_EDIT_KNN_CHUNK_SLOTS", "D2G_INTERVAL_LIST_POSITIONS", "D2G_SCREEN_RESULT_PAIRS", "D2G_EDIT_GRID_MAX",
            "D2G_EDIT_DEDUP_CHUNK", "D2G_EDIT_DEDUP_MAX_CHUNKS")
DEFAULTS = {"D2G_KNN_CHUNK_SLOTS": 1 << 24, "D2G_EDIT_KNN_CHUNK_SLOTS": 1 << 24, "D2G_INTERVAL_LIST_POSITIONS": 0, "D2G_SCREEN_RESULT_PAIRS": 1 << 30,
            "D2G_EDIT_GRID_MAX": (1 << 31) - 1, "D2G_EDIT_DEDUP_CHUNK": 1024, "D2G_EDIT_DEDUP_MAX_CHUNKS": 1024}


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


def div_up(a, b):
    return (a + b - 1) // b


def resolved(ctx, name):
    return int(ctx.tuning()["resolved"][name])


def unswitched(ctx, monkeypatch):
    for name in SWITCHES:
        monkeypatch.delenv(name, raising=False)
    assert {n: resolved(ctx, n) for n in SWITCHES} == DEFAULTS


class Launches:
    """the launches kernel_ms logs under `names` while the block runs -> .n[name]"""
    def __init__(self, ctx, flags, *names):
        self.ctx, self.flags, self.names, self.n = ctx, flags, names, {}

    def __enter__(self):
        self.ctx.set_timing(self.flags)
        for name in self.names:
            self.ctx.kernel_ms(name)
        return self

    def __exit__(self, *exc):
        for name in self.names:
            self.n[name] = self.ctx.kernel_ms(name)[0]
        self.ctx.set_timing(0)


def same_bits(a, b):
    return all(x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes() for x, y in zip(a, b))


def test_an_unset_or_invalid_switch_resolves_to_the_constant(gpu_ctx, monkeypatch):
    unswitched(gpu_ctx, monkeypatch)
    for name in SWITCHES:
        for bad in ("0", "-1", "12x", "", "99999999999999999999999"):
            monkeypatch.setenv(name, bad)
            assert resolved(gpu_ctx, name) == DEFAULTS[name], (name, bad)
        monkeypatch.delenv(name)
    monkeypatch.setenv("D2G_EDIT_DEDUP_CHUNK", "300")                                  # not a multiple of the workgroup
    monkeypatch.setenv("D2G_EDIT_DEDUP_MAX_CHUNKS", "1025")
    monkeypatch.setenv("D2G_SCREEN_RESULT_PAIRS", str((1 << 30) + 1))
    monkeypatch.setenv("D2G_EDIT_GRID_MAX", str(1 << 31))
    assert {n: resolved(gpu_ctx, n) for n in SWITCHES} == DEFAULTS
    monkeypatch.setenv("D2G_EDIT_GRID_MAX", "7")
    assert resolved(gpu_ctx, "D2G_EDIT_GRID_MAX") == 7 and gpu_ctx.tuning()["D2G_EDIT_GRID_MAX"] == "7"


# ---------------------------------------------------------------- 1. d2g_cmp_set_knn: chunks of rows, re-run groups
def knn_cap(K, cap, N):
    return min(cap if cap else (max(2 * K, K + 32) if K else 64), max(N - 1, 1))


@pytest.mark.parametrize("kind,N", [("families", 257), ("identical", 257), ("duplicates", 257), ("families", 67)])
def test_knn_chunks_and_rerun_groups(gpu_ctx, d2g, oracle, monkeypatch, kind, N):
    """D2G_KNN_CHUNK_SLOTS in {1, 10 cap, 1000}: one row per chunk; ten; a chunk length that depends on the cap.  `identical`: every row
    overflows any cap below N - 1, and a re-run group's widest list times its rows must stay in the budget, so the groups are cut by it
    (below 2 (N - 1) slots: every row alone); `duplicates`: the copies of row 0 overflow cap = 1 between rows that fit, inside a chunk
    and on both sides of a chunk border (32 | 33 at chunks of 33 rows, 63 | 64 at chunks of 64)"""
    m = matrix(kind, N, 128)
    bits = m.sigs.view(np.uint64)
    modes = [dict(K=1, cap=0), dict(K=5, cap=7), dict(K=N + 10, cap=0), dict(K=1, cap=1), dict(K=4, cap=2, r0=9, r1=N - 5)]
    for measure, isdist in ((d2g.SIMILARITY, False), (d2g.POISSON_LLR, True)):
        v = oracle_values(oracle, m, measure)
        T = ((0.3 if kind == "families" else 1.0) if not isdist else (0.05 if kind == "families" else 1e-30))
        for mode in modes + [dict(threshold=T, cap=3)]:
            r0, r1 = mode.get("r0", 0), mode.get("r1", N)
            rows, K = r1 - r0, mode.get("K", 0)
            exp = KR.knn_intended(v, K=K or None, T=None if K else T, isdist=isdist, rows=(r0, r1))
            cap = knn_cap(K, mode["cap"], N)
            cnt = np.diff(exp[0].astype(np.int64))                                    # a row's count on the device is the length of its list
            if kind == "identical":
                assert (cnt == N - 1).all()
            unswitched(gpu_ctx, monkeypatch)
            with Launches(gpu_ctx, d2g.TIME_KNN, "knn") as plain:
                first = gpu_ctx.cmp_knn(bits, measure=measure, k=31, **mode)
            KR.assert_csr_equal(first, exp, f"{kind} measure {measure} {mode} no switch")
            # (1000 slots are one chunk where the cap is small; cap = 1: chunk borders at 32 | 33 and at 63 | 64, between copies of row 0)
            for slots in (1, 10 * cap) + ((1000,) if 1000 // cap < rows else ()) + ((33, 64) if mode == dict(K=1, cap=1) else ()):
                monkeypatch.setenv("D2G_KNN_CHUNK_SLOTS", str(slots))
                assert resolved(gpu_ctx, "D2G_KNN_CHUNK_SLOTS") == slots
                with Launches(gpu_ctx, d2g.TIME_KNN, "knn") as cut:
                    got = gpu_ctx.cmp_knn(bits, measure=measure, k=31, **mode)
                what = f"{kind} measure {measure} {mode} slots {slots}"
                KR.assert_csr_equal(got, exp, what)
                assert same_bits(got, first), what
                chunk = min(rows, max(1, slots // cap))
                chunks = div_up(rows, chunk)
                # a launch per chunk and one per re-run group: a chunk with an overflowed row has at least one, and two lists of N - 1
                # entries share a group only under a budget of 2 (N - 1) slots
                least = chunks + sum(1 for c in range(chunks) if (cnt[c * chunk:(c + 1) * chunk] > cap).any())
                if kind == "identical" and cap < N - 1 and slots < 2 * (N - 1):
                    least = chunks + rows
                assert chunks > 1 and cut.n["knn"] >= least and cut.n["knn"] > plain.n["knn"], (what, chunks, least, cut.n, plain.n)
    if kind == "duplicates":
        dup = KR.knn_intended(oracle_values(oracle, m, d2g.SIMILARITY), K=1)
        n = np.diff(dup[0].astype(np.int64))
        assert n[32] > 1 and n[33] > 1 and n[63] > 1 and n[64] > 1 and n[31] <= 1 and n[34] <= 1 and n[62] <= 1 and n[65] <= 1


# ---------------------------------------------------------------- 2. d2g_edit_knn: chunks at every level of the escalation
@pytest.mark.parametrize("mode", [dict(K=0, T=2), dict(K=0, T=31), dict(K=1, T=0), dict(K=1, T=1), dict(K=3, T=0), dict(K=3, T=1),
                                  dict(K="N+5", T=0), dict(K="N+5", T=1)], ids=lambda m: f"K{m['K']}-T{m['T']}")
def test_edit_knn_chunks_at_every_level(gpu_ctx, d2g, monkeypatch, mode):
    """D2G_EDIT_KNN_CHUNK_SLOTS in {1, 3 cap, 500} on the 70 records of the seam family.  Threshold mode: rows that fit and rows that
    overflow a small cap.  Top-K from the bounds 0 and 1: the rows short of K entries go on with 2 bound + 1 and are chunked again
    there, between rows of the same chunk that are complete or overflowed; the device buffers are shared by all levels"""
    recs, d = EC.seam_family()
    n = len(recs)
    K, T = (n + 5 if mode["K"] == "N+5" else mode["K"]), mode["T"]
    lists, _ = W.within_lists(recs, K, T, d)
    nnz = sum(map(len, lists))
    assert 0 < nnz and (nnz < n * (n - 1) or K >= n - 1)
    ss = gpu_ctx.seqset(recs)
    try:
        for small in (0, 2 if K == 0 else K if K <= 3 else 4):
            cap = knn_cap(K, small, n)
            unswitched(gpu_ctx, monkeypatch)
            with Launches(gpu_ctx, d2g.TIME_KNN, "knn") as plain:
                first = ss.knn(K=K, T=T, cap=small)
            assert_csr(first, lists, d)
            if small:
                assert max(map(len, lists)) > cap, "no row overflows the small cap"
            for slots in (1, 3 * cap) + (() if small else (500,)):
                monkeypatch.setenv("D2G_EDIT_KNN_CHUNK_SLOTS", str(slots))
                assert resolved(gpu_ctx, "D2G_EDIT_KNN_CHUNK_SLOTS") == slots
                with Launches(gpu_ctx, d2g.TIME_KNN, "knn") as cut:
                    got = ss.knn(K=K, T=T, cap=small)
                what = f"K {K} T {T} cap {small} slots {slots}"
                assert_csr(got, lists, d)
                assert same_bits(got, first), what
                chunks = div_up(n, max(1, slots // cap))
                assert chunks > 1 and cut.n["knn"] >= chunks and cut.n["knn"] > plain.n["knn"], (what, chunks, cut.n, plain.n)
        # a row range that starts inside a chunk of the whole set
        monkeypatch.setenv("D2G_EDIT_KNN_CHUNK_SLOTS", str(3 * knn_cap(K, 0, n)))
        assert_csr(ss.knn(K=K, T=T, r0=11, r1=30), lists, d, 11, 30)
    finally:
        ss.close()
    if K:                                                                            # the escalation is there to enter: rows that are short at the start ...
        at_start = [sum(1 for j in range(n) if j != i and d[i, j] <= T) for i in range(n)]
        assert any(c < min(K, n - 1) for c in at_start)
        if (K, T) in ((1, 0), (1, 1), (3, 1)):                                       # ... between rows that are not
            assert any(c >= K for c in at_start)


# ---------------------------------------------------------------- 3. d2g_interval_bmh_sketch: groups of files
_BMH = {}


def bmh_expected(oracle, name, buf, S, normalize):
    """(registers as bits or None for a file that covers nothing, total weight, covered positions) of one file: the reference's
    dictionary into the oracle's BagMinHash"""
    key = (name, S, normalize)
    if key not in _BMH:
        h, a, b, off = B.tables([buf])
        ids, ws, total = B.multiset_lists(list(zip(h.tolist(), a.tolist(), b.tolist())), normalize)
        sig = oracle.bmh_from_weighted(ids, ws, S)[0].view(np.uint64).copy() if ids.size else None
        _BMH[key] = (sig, total, int(ids.size))
    return _BMH[key]


def groups_of(covered, budget):
    """how many groups the files make, stated from the rule: files in order, a group is closed by the first file that would pass the budget"""
    n, used = 1, 0
    for c in covered:
        assert c <= budget
        if used + c > budget:
            n, used = n + 1, 0
        used += c
    return n


ORDERS = {
    "as-listed": ["depths", "dups", "empty", "norm", "norm-reordered", "high", "long"],
    "empty-first-and-last": ["empty", "depths", "dups", "long", "norm", "norm-reordered", "high", "empty"],
    # every file that covers something alone in its group under the budget of `long`, the files that cover nothing at both ends of a group
    "alone-1": ["empty", "depths", "empty", "long", "dups", "empty"],
    "alone-2": ["norm", "long", "norm-reordered"],
    "alone-3": ["high", "long", "empty"],
}


@pytest.mark.parametrize("normalize", [False, True], ids=["counts", "normalized"])
@pytest.mark.parametrize("S", [64, 100])
@pytest.mark.parametrize("order", list(ORDERS))
def test_interval_groups_of_files(gpu_ctx, d2g, oracle, monkeypatch, order, S, normalize):
    """D2G_INTERVAL_LIST_POSITIONS = the covered positions of the largest file (it must pass, alone), a budget that packs several small
    files per group, and the largest file minus one position: D2G_ERR_NOMEM with the bytes it needs, nothing outside the outputs written"""
    files = _ms_files()
    names = ORDERS[order]
    exp = [bmh_expected(oracle, name, files[name], S, normalize) for name in names]
    covered = [e[2] for e in exp]
    largest = max(covered)
    assert largest == 8000 and covered[names.index("long")] == 8000
    if order == "as-listed":
        assert covered == [400, 125, 0, 14, 14, 80, 8000]
    h, a, b, off = B.tables([files[name] for name in names])
    p = gpu_ctx.interval_plan(h, a, b, off)

    def check(sig, tw, what):
        for f, (esig, etw, _) in enumerate(exp):
            assert tw[f] == etw, (what, names[f])
            if esig is None:
                assert np.isinf(sig[f]).all() and tw[f] == 0., (what, names[f])
            else:
                assert np.array_equal(sig[f].view(np.uint64), esig), (what, names[f])

    try:
        unswitched(gpu_ctx, monkeypatch)
        with Launches(gpu_ctx, True, "k1iexpand", "k1ibmh") as plain:
            first = gpu_ctx.interval_bmh_sketch(p, S, normalize=normalize)
        check(*first, "no switch")
        assert plain.n == {"k1iexpand": 1, "k1ibmh": 1}
        # (a budget below the largest file fails.)  + 28: `long` takes both `norm` files along where they follow it; + 107: `high` too
        budgets = [largest] + ([] if order.startswith("alone") else [largest + 28, largest + 107])
        for budget in budgets:
            monkeypatch.setenv("D2G_INTERVAL_LIST_POSITIONS", str(budget))
            assert resolved(gpu_ctx, "D2G_INTERVAL_LIST_POSITIONS") == budget
            with Launches(gpu_ctx, True, "k1iexpand", "k1ibmh") as cut:
                got = gpu_ctx.interval_bmh_sketch(p, S, normalize=normalize)
            check(*got, f"budget {budget}")
            assert same_bits(got, first)
            ng = groups_of(covered, budget)
            assert ng > 1 and cut.n["k1ibmh"] == ng and cut.n["k1iexpand"] == ng, (budget, ng, cut.n)
            if order.startswith("alone"):
                assert ng == sum(1 for c in covered if c)
            elif budget == largest:
                assert ng == (2 if order == "as-listed" else 3)                      # the six small files and `long`; three files, `long`, four files
        # one position short of the largest file
        monkeypatch.setenv("D2G_INTERVAL_LIST_POSITIONS", str(largest - 1))
        guard, n = 16, len(names)
        sig = np.full(2 * guard + n * S, -7.25, np.float64)
        tw = np.full(2 * guard + n, -7.25, np.float64)
        rc = d2g.lib().d2g_interval_bmh_sketch(gpu_ctx._h, p._h, int(normalize), S, ctypes.c_void_p(sig.ctypes.data + 8 * guard),
                                                      ctypes.c_void_p(tw.ctypes.data + 8 * guard))
        msg = d2g.lib().d2g_last_error(gpu_ctx._h).decode()
        assert rc == ERR_NOMEM and f"need {16 * largest} bytes" in msg and "D2G_INTERVAL_LIST_POSITIONS" in msg and str(16 * (largest - 1)) in msg, (rc, msg)
        for arr in (sig, tw):
            assert (arr[:guard] == -7.25).all() and (arr[-guard:] == -7.25).all(), "guard words around an output were written"
        at = names.index("long")
        assert (sig[guard + at * S:] == -7.25).all() and (tw[guard + at:] == -7.25).all()   # nothing from the file that failed on
    finally:
        p.close()


# ---------------------------------------------------------------- 4. d2g_screen_result: passes of whole rows
@pytest.fixture(scope="module")
def screened(d2g, gpu_ctx):
    """the database of test_gpu_screen.py's family (k = 21, three references sketched from a 4000-base genome, S = 64) and seven rows
    of reads from it, one of them without a k-mer; the rows' expected results by contain_ref's closed form"""
    rng = np.random.default_rng(2121)
    g = KC.random_bases(rng, 4000)
    other = KC.random_bases(rng, 2000)
    refs = [[g[:2500]], [g[1500:]], [other]]
    db = OK.decode(np.stack([OK.genome_closed_form(r, 21, True, 0, 64)[0] for r in refs])[:, :64])
    rows = [[g[200:1200]], [g[1400:1700], g[1500:1600]], ["ACGTACGT"], [g[3000:4000]], [KC.random_bases(np.random.default_rng(77), 1500), other[100:900]],
            [g[:150], g[2400:2600]], [g[100:3900]]]
    want = [CR.closed_form(db, *KC.key_counts(tuple(r), 21, True, 0)[:2]) for r in rows]
    em, es = np.stack([w[0] for w in want]).astype(np.uint32), np.stack([w[1] for w in want]).astype(np.uint32)
    assert len({tuple(r) for r in em.tolist()}) == 7 and not em[2].any() and (em > 0).any(0).all() and (es > em).any()
    return db, rows, em, es


def test_screen_result_in_passes(gpu_ctx, d2g, screened, monkeypatch):
    """D2G_SCREEN_RESULT_PAIRS in {1, 2 nrefs, 3 nrefs + 1}: one, two and three rows per pass over seven rows and over rows [2, 7): the
    last pass is ragged, the second half of the device buffer starts at rows_per x nrefs"""
    db, rows, em, es = screened
    nrefs = db.shape[0]
    sc = gpu_ctx.screen(db, 21, canon=True, xormask=0, nrows=len(rows))
    sk = gpu_ctx.sketcher()
    try:
        sk.run_screen(pack(d2g, 21, rows), sc, list(range(len(rows))), canon=True)
        for row0, nrows in ((0, 7), (2, 5), (6, 1)):
            unswitched(gpu_ctx, monkeypatch)
            with Launches(gpu_ctx, d2g.TIME_SCREEN, "screenreduce") as plain:
                first = sc.result(row0, nrows)
            assert plain.n["screenreduce"] == 1
            np.testing.assert_array_equal(first[0], em[row0:row0 + nrows])
            np.testing.assert_array_equal(first[1], es[row0:row0 + nrows])
            for pairs in (1, 2 * nrefs, 3 * nrefs + 1):
                monkeypatch.setenv("D2G_SCREEN_RESULT_PAIRS", str(pairs))
                assert resolved(gpu_ctx, "D2G_SCREEN_RESULT_PAIRS") == pairs
                with Launches(gpu_ctx, d2g.TIME_SCREEN, "screenreduce") as cut:
                    got = sc.result(row0, nrows)
                np.testing.assert_array_equal(got[0], em[row0:row0 + nrows], err_msg=f"matches, rows {row0, nrows} pairs {pairs}")
                np.testing.assert_array_equal(got[1], es[row0:row0 + nrows], err_msg=f"matchsums, rows {row0, nrows} pairs {pairs}")
                assert same_bits(got, first)
                rows_per = max(1, min(nrows, pairs // nrefs))
                assert cut.n["screenreduce"] == div_up(nrows, rows_per)
                if nrows > 1:
                    assert cut.n["screenreduce"] > 1 and (pairs == 1 or nrows % rows_per)
    finally:
        sk.close(); sc.close()


# ---------------------------------------------------------------- 5. the edit-distance launches: rows per launch
LAUNCH_TILES = (512, 64, 8)                                                          # column records per workgroup of the three row classes


def edit_pieces(ctx, rows, ncols, tile=None):
    """the launches of one row class: rows / max(1, grid max / tiles) -- the fewest over the classes"""
    grid_max = resolved(ctx, "D2G_EDIT_GRID_MAX")
    return min(div_up(rows, max(1, grid_max // div_up(ncols, t))) for t in ((tile,) if tile else LAUNCH_TILES))


@pytest.mark.parametrize("tile,grid_max", [(None, 1), (None, 5), (None, 7), (3, 20), (3, 30)])
def test_edit_rows_per_launch(gpu_ctx, torch, monkeypatch, tile, grid_max):
    """D2G_EDIT_GRID_MAX: launches whose first row is not the call's, in all three row classes (records of at most 8 blocks, of one
    strip, of several), for the triangle's index, the rectangle's and the host-pointer forms"""
    recs, want = seam_set()
    n = len(recs)
    blocks = [(len(r) + 31) // 32 for r in recs[4:31]]
    assert min(blocks) <= 8 and any(8 < b <= 64 for b in blocks) and max(blocks) > 64      # rows [4, 31) hold all three classes
    if tile:
        monkeypatch.setenv("D2G_EDIT_TILE", str(tile))
    ss = gpu_ctx.seqset(recs)
    try:
        def run():
            return (ut_of(gpu_ctx, torch, ss, 4, 31), rect_of(gpu_ctx, torch, ss, 2, 40, 1, 33), ss.edit_ut().astype(np.int64),
                    ss.edit_rect(3, 19, 0, n).astype(np.int64), ut_of(gpu_ctx, torch, ss), rect_of(gpu_ctx, torch, ss, 0, n, 0, n))

        monkeypatch.delenv("D2G_EDIT_GRID_MAX", raising=False)
        assert resolved(gpu_ctx, "D2G_EDIT_GRID_MAX") == DEFAULTS["D2G_EDIT_GRID_MAX"]
        first = run()
        monkeypatch.setenv("D2G_EDIT_GRID_MAX", str(grid_max))
        for rows in (27, 38, n, 16):
            assert edit_pieces(gpu_ctx, rows, n, tile) > 1
        got = run()
        for g, w in zip(got, (E.triangle(want, 4, 31), want[2:40, 1:33], E.triangle(want), want[3:19], E.triangle(want), want)):
            np.testing.assert_array_equal(g, w)
        assert same_bits(got, first)
    finally:
        ss.close()


@pytest.mark.parametrize("T", [2, 31, 40])
@pytest.mark.parametrize("tile,grid_max", [(None, 1), (None, 5), (3, 20), (3, 30)])
def test_edit_near_rows_per_launch(gpu_ctx, torch, d2g, monkeypatch, T, tile, grid_max):
    """d2g_edit_near_dev under D2G_EDIT_GRID_MAX: T = 2 and 31 the band kernel's launches (D2G_EDIT_NEAR_ROUTE=1 makes the whole call
    one run of rows, so that its piece count follows from the shape; the dispatcher's own runs are checked beside it), T = 40 the pair
    kernel over the window of the order, where the kernel's N is the window"""
    recs, d = seam_set()
    n = len(recs)
    want = W.closeness(d, T)
    assert 0 < int((want > 0).sum()) - n < n * (n - 1)
    if tile:
        monkeypatch.setenv("D2G_EDIT_TILE", str(tile))
    ss = gpu_ctx.seqset(recs)
    try:
        for route in (0, 1) if T <= 31 else (0,):
            monkeypatch.setenv("D2G_EDIT_NEAR_ROUTE", str(route))
            monkeypatch.delenv("D2G_EDIT_GRID_MAX", raising=False)
            first = (near_of(gpu_ctx, torch, ss, T), near_of(gpu_ctx, torch, ss, T, 4, 31))
            monkeypatch.setenv("D2G_EDIT_GRID_MAX", str(grid_max))
            with Launches(gpu_ctx, d2g.TIME_EDIT_NEAR | d2g.TIME_EDIT, "editnear", "edit") as cut:
                got = (near_of(gpu_ctx, torch, ss, T), near_of(gpu_ctx, torch, ss, T, 4, 31))
            np.testing.assert_array_equal(got[0], want, err_msg=f"route {route}")
            np.testing.assert_array_equal(got[1], want[4:31], err_msg=f"route {route}, rows [4, 31)")
            assert same_bits(got, first)
            if T > 31:                                                               # one run of rows per call: the pair kernel and the clamp
                assert cut.n == {"editnear": 2, "edit": 2}
                lens = np.array([len(r) for r in recs])

                def window(r0, r1):                                                  # the columns whose length is within T of a row's
                    return int(((lens >= lens[r0:r1].min() - T) & (lens <= lens[r0:r1].max() + T)).sum())

                assert window(0, n) == n and 1 < window(4, 31) < n                   # the kernel's N is the window, not the set
                assert edit_pieces(gpu_ctx, 27, window(4, 31), tile) > 1 and edit_pieces(gpu_ctx, n, n, tile) > 1
            elif route == 1:                                                         # one run, the band kernel alone: tiles of 512 positions
                assert cut.n == {"editnear": 2, "edit": 0}
                rows_per = max(1, grid_max // div_up(n, tile or 512))
                assert div_up(n, rows_per) > 1 and div_up(27, rows_per) > 1
    finally:
        ss.close()


# ---------------------------------------------------------------- 6, 7. d2g_edit_dedup_dev: the compaction's workgroups
def compaction(ctx, n):
    """(positions per workgroup, workgroups) of the compaction over n records, from the resolved switches"""
    base, most = resolved(ctx, "D2G_EDIT_DEDUP_CHUNK"), resolved(ctx, "D2G_EDIT_DEDUP_MAX_CHUNKS")
    chunk = max(base, div_up(div_up(n, most), 256) * 256)
    return chunk, div_up(n, chunk)


def short_duplicates():
    """2500 records of 5 to 7 DNA symbols drawn from 1500 distinct strings, shuffled.  At T = 0 two records are within the bound iff they
    are equal: a record's representative is the first index that holds its bytes -- known by construction"""
    rng = np.random.default_rng(2500)
    pool = set()
    while len(pool) < 1500:
        pool.add(bytes(rng.choice(EC.DNA, int(rng.integers(5, 8))).tolist()))
    pool = sorted(pool)
    recs = [pool[i] for i in rng.permutation(1500)] + [pool[int(i)] for i in rng.integers(0, 1500, 1000)]
    recs = [recs[i] for i in rng.permutation(2500)]
    seen = {}
    want = np.array([seen.setdefault(r, i) for i, r in enumerate(recs)], np.uint32)
    return recs, want


def test_edit_dedup_representatives_across_compaction_workgroups(gpu_ctx, torch, d2g, monkeypatch):
    """no switch: 2500 records are three compaction workgroups of 1024 positions of the order by length, which is not the input order; a
    workgroup's representatives go behind the sum of the earlier workgroups' counts.  1500 representatives: the first and the second
    workgroup hold representatives at the latest from the band on that sees 1024 / 2048 of them"""
    recs, want = short_duplicates()
    n = len(recs)
    reps = np.flatnonzero(want == np.arange(n))
    assert reps.size == 1500 and len(set(map(len, recs))) == 3
    lens = np.array([len(r) for r in recs])
    order = np.argsort(lens, kind="stable")
    assert (np.diff(order) < 0).any()
    unswitched(gpu_ctx, monkeypatch)
    assert compaction(gpu_ctx, n) == (1024, 3)
    isrep = want[order] == order
    assert all(isrep[c:c + 1024].sum() > 100 for c in (0, 1024, 2048))                 # every workgroup has many to place
    ss = gpu_ctx.seqset(recs)
    try:
        for route in (0, 1, 2):
            for reverse in (0, 1):
                for band_rows in (0, 100):
                    monkeypatch.setenv("D2G_EDIT_DEDUP_ROUTE", str(route))
                    monkeypatch.setenv("D2G_EDIT_DEDUP_REVERSE", str(reverse))
                    with Launches(gpu_ctx, d2g.TIME_EDIT_DEDUP, "editdedup_list") as cut:
                        got = dedup_of(gpu_ctx, torch, ss, 0, band_rows)
                    np.testing.assert_array_equal(got, want, err_msg=f"route {route} reverse {reverse} band_rows {band_rows}")
                    assert cut.n["editdedup_list"] == div_up(n, band_rows or 256)     # a compaction per band, each of three workgroups
    finally:
        ss.close()


@pytest.mark.parametrize("T", [1, 2])
@pytest.mark.parametrize("chunk,most,geometry", [(256, None, (256, 3)), (256, 2, (512, 2)), (256, 1, (768, 1))],
                         ids=["three-of-256", "two-of-512", "one-of-768"])
def test_edit_dedup_compaction_chunk_sizes(gpu_ctx, torch, d2g, monkeypatch, T, chunk, most, geometry):
    """D2G_EDIT_DEDUP_CHUNK / D2G_EDIT_DEDUP_MAX_CHUNKS on the 513 records of the band family: three workgroups of 256 positions; two of
    512 (two rounds of the workgroup each); one that walks 768 positions, more than a workgroup's share under the switch, as a set above
    2^20 records makes every workgroup do"""
    recs, d = EC.band_family()
    n = len(recs)
    want = np.asarray(ER.greedy_assign(d, T), np.uint32)
    assert 1 < ER.n_clusters(want) < n
    ss = gpu_ctx.seqset(recs)
    try:
        for route in (0, 1, 2):
            unswitched(gpu_ctx, monkeypatch)
            monkeypatch.setenv("D2G_EDIT_DEDUP_ROUTE", str(route))
            assert compaction(gpu_ctx, n) == (1024, 1)
            first = dedup_of(gpu_ctx, torch, ss, T)
            monkeypatch.setenv("D2G_EDIT_DEDUP_CHUNK", str(chunk))
            if most:
                monkeypatch.setenv("D2G_EDIT_DEDUP_MAX_CHUNKS", str(most))
            assert compaction(gpu_ctx, n) == geometry
            assert geometry[1] > 1 or geometry[0] > resolved(gpu_ctx, "D2G_EDIT_DEDUP_CHUNK")
            for reverse in (0, 1):
                monkeypatch.setenv("D2G_EDIT_DEDUP_REVERSE", str(reverse))
                with Launches(gpu_ctx, d2g.TIME_EDIT_DEDUP, "editdedup_list") as cut:
                    got = dedup_of(gpu_ctx, torch, ss, T, 100 if reverse else 0)
                np.testing.assert_array_equal(got, want, err_msg=f"route {route} reverse {reverse}")
                assert got.tobytes() == first.tobytes()
                assert cut.n["editdedup_list"] == div_up(n, 100 if reverse else 256)
            monkeypatch.delenv("D2G_EDIT_DEDUP_REVERSE")
    finally:
        ss.close()
