"""The multi-GPU engine (d2g_mgpu.hip) over the loopback transport with EVERY RANK ON ITS OWN STREAM and A NEW MATRIX EVERY STEP.

test_gpu_mgpu.py drives the W contexts of device 0 with streams == NULL, so every rank's pack, prepare, derive, order and pair kernel go to
the one legacy default stream and queue order alone does what the engine's fences (ev_pack, ev_x1[c], ev_prep[c], ev_x2[c], the ready / done
pair of the loopback copies) must do between real devices; and it repeats its steps on the same rows, so anything stale -- a receive chunk,
a block of plane groups with its meta and status word, an exporter set's ids, a pre-filled slab -- gives last step's answer, the right one.
Here each rank has a torch stream of its own, the ranks are thrown out of step with each other by ballast on every other rank's stream, the
rows are copied into ONE reused buffer per rank on that stream right before the call, and the matrices are those of mgpu_stream_cases.py:
consecutive ones share no 64-bit pattern, and every 32-register group changes the counts of every rank's slab (P1-P3 there, checked on the
CPU by test_mgpu_stream_cases.py).  Expected values are the oracle's; every comparison is exact; every output starts as a pattern no result
contains and has guard words behind it.

This is as far as one GPU goes: it proves the ordering and the reuse of buffers, not RCCL, which has run with one rank only."""
import numpy as np
import pytest

import mgpu_stream_cases as M
from gpu_ballast import keep_busy

pytestmark = pytest.mark.gpu

GUARD = 64                                                            # 32-bit words behind every output
FILL = 0xABABABAB                                                     # no count (<= S) and no table value used here has these bits


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


class Slab:
    """a device output of n 32-bit words with GUARD words behind it, every word = FILL"""

    def __init__(self, torch, n):
        self.n = n
        self.t = torch.full((n + GUARD,), FILL - (1 << 32), dtype=torch.int32, device="cuda")

    @property
    def ptr(self):
        return self.t.data_ptr()

    def words(self, t=None):
        """the n words on the host (of a clone, if one is given); the guard words must be as they were"""
        host = (self.t if t is None else t).cpu().numpy().view(np.uint32)
        assert (host[self.n:] == FILL).all(), "the guard words behind an output were written"
        return host[:self.n]

    def assert_untouched(self):
        assert (self.words() == FILL).all(), "a refused call wrote to its output"


class Group:
    """W contexts on device 0 (created NOW: they read the D2G_* switches of this moment), their loopback communicators and engines, one
    torch stream per rank, one reused rows buffer per rank"""

    def __init__(self, d2g, torch, W, N, S):
        self.d2g, self.torch, self.W, self.N, self.S = d2g, torch, W, N, S
        self.ctxs = [d2g.Context(0) for _ in range(W)]
        self.comms = d2g.Comm.create_all(self.ctxs)
        assert not any(c.is_rccl for c in self.comms)
        self.engs = [d2g.AllPairs(self.ctxs[r], self.comms[r], N, S) for r in range(W)]
        self.streams = [torch.cuda.Stream() for _ in range(W)]
        self.sp = [s.cuda_stream for s in self.streams]
        self.held = [e.rows_held for e in self.engs]
        assert [h[0] for h in self.held] + [N] == M.even_split(N, W)
        b = d2g.ut_partition(N, W)
        assert [e.rows_computed for e in self.engs] == [(b[r], b[r + 1]) for r in range(W)]
        self.off = M.ut_offsets(N)
        self.cnt = [d2g.ut_count(N, *e.rows_computed) for e in self.engs]
        self.rows = [torch.zeros((hi - lo, S), dtype=torch.int64, device="cuda") for lo, hi in self.held]

    def stage(self, m):
        """every rank's rows of one matrix on the device (not yet in the rows buffers)"""
        bits = np.ascontiguousarray(m).view(np.int64)
        return [self.torch.from_numpy(bits[lo:hi]).cuda() for lo, hi in self.held]

    def feed(self, staged, t):
        """on every rank's stream: ballast if (rank + t) is odd, then the rank's rows into its reused buffer"""
        for r in range(self.W):
            with self.torch.cuda.stream(self.streams[r]):
                if (r + t) % 2:
                    keep_busy(self.torch)
                self.rows[r].copy_(staged[r])

    def step(self, luts, outs):
        self.d2g.allpairs_step_all(self.engs, [x.data_ptr() for x in self.rows], None if luts is None else [x.data_ptr() for x in luts],
                                   [o.ptr for o in outs], self.sp)

    def clones(self, outs):
        """every rank's output cloned on the rank's stream, behind its pair kernel"""
        got = []
        for r in range(self.W):
            with self.torch.cuda.stream(self.streams[r]):
                got.append(outs[r].t.clone())
        return got

    def slabs(self):
        return [Slab(self.torch, n) for n in self.cnt]

    def expected(self, exp, r, lut=None):
        r0, r1 = self.engs[r].rows_computed
        e = exp[self.off[r0]:self.off[r1]]
        return e if lut is None else lut[e].view(np.uint32)

    def assert_clean(self):
        for r, e in enumerate(self.engs):
            e.status(self.sp[r])

    def close(self):
        self.torch.cuda.synchronize()
        for x in self.engs + self.comms + self.ctxs:
            x.close()


def _tables(d2g, torch, S, W):
    """name -> (host table, one device copy per rank): SIMILARITY (lut[0] == 0) and a table whose value for "no register equal" is not 0"""
    sim = d2g.epilogue_lut(S, d2g.SIMILARITY, 31, multiset_space=bool(S & (S - 1)))   # (the set-space table exists for powers of two only)
    plus7 = (np.arange(S + 1) + 7).astype(np.float32)
    assert sim[0] == 0 and plus7[0] != 0 and sim.dtype == np.float32
    return {k: (v, [torch.from_numpy(v).cuda() for _ in range(W)]) for k, v in (("sim", sim), ("plus7", plus7))}


# ---------------------------------------------------------------- 1. a stream of matrices, no host synchronisation between the steps
FORMS = (None, "sim", "plus7")                                        # step t runs FORMS[t % 3]: u32 counts, a table with lut[0] == 0, one with lut[0] != 0
REUSE = {4: 0}                                                        # step 4 (a table step) writes into the buffer step 0 (counts) used


@pytest.mark.parametrize("W,N,S,chunks", [(2, 263, 1000, None), (3, 517, 96, "1"), (4, 300, 1024, "4"), (8, 77, 1024, "2"), (5, 129, 100, None)])
def test_stream_of_matrices_on_per_rank_streams(d2g, oracle, torch, monkeypatch, W, N, S, chunks):
    """T = 6 planted matrices through one group, enqueued back to back: for step t, on rank r's stream, ballast if (r + t) is odd, the
    rank's rows of M_t into its ONE rows buffer, then one d2g_allpairs_step_all for all ranks, then a clone of every rank's output on its
    stream.  The steps alternate between u32 counts and two float tables; step 4 writes its table values into the buffer step 0's counts
    were cloned from.  ONE synchronisation, after the last enqueue; then every rank's whole slab of every step against the oracle."""
    assert (W, N, S) in M.STREAM_SHAPES
    if chunks is not None:
        monkeypatch.setenv("D2G_MGPU_CHUNKS", chunks)
    T = M.STREAM_T
    mats = M.sequence(N, S, T, M.seed_of(W, N, S), M.PLANTED_KINDS)
    exps = [oracle.eqcounts_ut(m) for m in mats]
    g = Group(d2g, torch, W, N, S)
    if chunks is not None:
        assert [e.chunks for e in g.engs] == [int(chunks)] * W
    tabs = _tables(d2g, torch, S, W)
    staged = [g.stage(m) for m in mats]
    outs = [g.slabs() for _ in range(T)]
    torch.cuda.synchronize()
    got = []
    for t in range(T):
        g.feed(staged[t], t)
        form = FORMS[t % 3]
        target = outs[REUSE.get(t, t)]
        g.step(None if form is None else tabs[form][1], target)
        got.append(g.clones(target))
    torch.cuda.synchronize()
    for t in range(T):
        form = FORMS[t % 3]
        for r in range(W):
            want = g.expected(exps[t], r, None if form is None else tabs[form][0])
            np.testing.assert_array_equal(outs[t][r].words(got[t][r]), want, err_msg=f"step {t} ({form or 'counts'}) rank {r}")
    for t in range(T):                                                # what the buffers hold at the end: the last step that wrote them, or the pattern
        writers = [u for u in range(T) if REUSE.get(u, u) == t]
        for r in range(W):
            if writers:
                np.testing.assert_array_equal(outs[t][r].words(), outs[t][r].words(got[writers[-1]][r]), err_msg=f"buffer {t} rank {r}")
            else:
                outs[t][r].assert_untouched()
    g.assert_clean()
    g.close()


# ---------------------------------------------------------------- 2. the sparse-tile path on the gathered operand, structure changing
@pytest.mark.parametrize("W,N,S", M.FAMILY_SHAPES)
def test_sparse_tiles_follow_a_changing_structure(d2g, oracle, torch, monkeypatch, W, N, S):
    """families -> one_family -> families -> planted(3) -> families ... for 18 steps, every rank on its own stream, three rounds per step
    (counts, table, counts: every round exchanges and orders again): every rank's whole slab against the oracle in every round, and the
    path d2g_allpairs_sparse_info reports.

    The path follows the set's documented memory (d2g.h, test_k2_sparse_give_up_is_remembered_per_set): an ordering that gives up -- one_family,
    planted(3): one root holds most sketches -- is remembered, the next prepares skip the ordering and walk densely, every 16th prepare of
    the set orders again.  So the model below says for EVERY round whether the ordering ran; a families round whose ordering ran must list
    tiles and use the pair list, exactly as test_allpairs_sparse_tiles_on_the_gathered_operand asks of its one matrix; a one_family round
    and every round that skipped must have run the dense kernel.  With three prepares a step the retry at the set's 32nd prepare falls
    into step 10, a families step behind a remembered give-up: the sparse path must come back there (asserted).

    Round 0 of a step is the one that meets a NEW matrix: it carries the evidence against stale state (18 of them).  Rounds 1 and 2 repeat
    the step's rows -- anything stale there gives the right answer -- and are here for the second epilogue and the count of prepares."""
    from concurrent.futures import ThreadPoolExecutor
    monkeypatch.setenv("D2G_BS_SPARSE_MIN_N", "1")
    monkeypatch.setenv("D2G_SP_TILE_FRAC", "1")                       # (matrices this small have few tiles: the families' share of them is large)
    T = M.FAMILY_T
    mats = M.sequence(N, S, T, M.seed_of(W, N, S), M.FAMILY_KINDS)
    with ThreadPoolExecutor(8) as pool:
        exps = list(pool.map(oracle.eqcounts_ut, mats))
    g = Group(d2g, torch, W, N, S)
    lut, luts = _tables(d2g, torch, S, W)["sim"]
    staged = [g.stage(m) for m in mats]
    outs = g.slabs()
    torch.cuda.synchronize()
    gave_up, prepares, came_back = [False] * W, 0, [False] * W
    for t in range(T):
        kind = M.FAMILY_KINDS[t % len(M.FAMILY_KINDS)]
        g.feed(staged[t], t)
        for rnd, use_lut in enumerate((False, True, False)):
            g.step(luts if use_lut else None, outs)
            prepares += 1
            for r in range(W):
                what = f"step {t} ({kind}) round {rnd} rank {r}"
                g.ctxs[r].sync(g.sp[r])
                g.engs[r].status(g.sp[r])
                np.testing.assert_array_equal(outs[r].words(), g.expected(exps[t], r, lut if use_lut else None), err_msg=what)
                info = g.engs[r].sparse_info()
                assert info["sorted_operand"], what
                assert info["ordering_skipped"] == (gave_up[r] and prepares % 16 != 0), (what, prepares, info)
                if info["ordering_skipped"]:
                    assert info["dense_kernel_ran"], (what, info)
                elif kind == "families":
                    assert info["tiles_listed"] > 0 and info["tiles_and_pair_list"] and not info["dense_decided_by_prepare"], (what, info)
                    came_back[r] |= gave_up[r]
                if kind == "one_family":
                    assert info["dense_kernel_ran"], (what, info)
                gave_up[r] = info["dense_decided_by_prepare"]
    assert all(came_back), "no families round behind a remembered give-up ran the ordering again"
    g.close()


# ---------------------------------------------------------------- 3. the CLI's pattern with a changing matrix
def test_prepare_all_then_batches_on_every_ranks_operand(d2g, oracle, torch):
    """d2g_allpairs_prepare_all on per-rank streams for M_0, M_1, M_2, no host synchronisation in between; after each prepare every rank
    launches on ITS stream, on ITS gathered operand, the row batches dealt to it round-robin (together the whole triangle) and one
    rectangle off the tile grid.  The union of the batches and every rectangle against the oracle of that step; what a rank was not dealt
    stays the fill pattern."""
    W, N, S = 4, 300, 1024
    assert (W, N, S) in M.STREAM_SHAPES
    BATCH = 37
    mats = M.sequence(N, S, 3, M.seed_of(W, N, S), M.PLANTED_KINDS)
    exps = [oracle.eqcounts_ut(m) for m in mats]
    g = Group(d2g, torch, W, N, S)
    staged = [g.stage(m) for m in mats]
    tri = [Slab(torch, N * (N - 1) // 2) for _ in range(W)]
    rect_of = [(1 + r, N // 2 - r, N // 3 + r, N - r) for r in range(W)]          # rows [a0, a1) x columns [b0, b1): no bound on a tile edge
    rects = [Slab(torch, (a1 - a0) * (b1 - b0)) for a0, a1, b0, b1 in rect_of]
    batches = [(a, min(a + BATCH, N)) for a in range(0, N, BATCH)]
    torch.cuda.synchronize()
    got_tri, got_rect = [], []
    for t in range(3):
        g.feed(staged[t], t)
        d2g.allpairs_prepare_all(g.engs, [x.data_ptr() for x in g.rows], g.sp)
        for r in range(W):
            op = g.engs[r].operand()
            for k, (a, b) in enumerate(batches):
                if k % W == r:
                    op.eqcount_ut_dev(tri[r].ptr + 4 * int(g.off[a]), a, b, stream=g.sp[r])
            op.eqcount_rect_dev(rects[r].ptr, *rect_of[r], stream=g.sp[r])
        got_tri.append(g.clones(tri))
        got_rect.append(g.clones(rects))
        for r in range(W):                                            # the next step starts from the pattern again
            with torch.cuda.stream(g.streams[r]):
                tri[r].t.fill_(FILL - (1 << 32))
                rects[r].t.fill_(FILL - (1 << 32))
    torch.cuda.synchronize()
    for t in range(3):
        full = np.zeros((N, N), np.uint32)
        full[np.triu_indices(N, 1)] = exps[t]
        full = full + full.T + np.diag(np.full(N, S, np.uint32))
        union = np.full(N * (N - 1) // 2, FILL, np.uint32)
        for r in range(W):
            host = tri[r].words(got_tri[t][r])
            mine = np.zeros(host.size, bool)
            for k, (a, b) in enumerate(batches):
                if k % W == r:
                    mine[g.off[a]:g.off[b]] = True
            assert (host[~mine] == FILL).all(), f"step {t} rank {r}: a batch wrote outside its rows"
            union[mine] = host[mine]
            a0, a1, b0, b1 = rect_of[r]
            np.testing.assert_array_equal(rects[r].words(got_rect[t][r]).reshape(a1 - a0, b1 - b0), full[a0:a1, b0:b1], err_msg=f"step {t} rank {r} rectangle")
        np.testing.assert_array_equal(union, exps[t], err_msg=f"step {t}")
    g.assert_clean()
    g.close()


# ---------------------------------------------------------------- 4. overflow, then a clean step on a different matrix
def test_refused_step_then_a_clean_step_on_another_matrix(d2g, oracle, torch, monkeypatch):
    """The D2G_BS_TAGBITS=0 arrangement of test_allpairs_status_reaches_every_rank on per-rank streams: rank 0's column slice overflows, both
    ranks report it; after d2g_ctx_reload_tuning the SAME engines run a step on a NEW matrix: every rank's whole slab is the oracle's and
    every status is clean -- nothing of the refused operand (planes, meta, status words) is left in the new one."""
    W, N, S = M.OVERFLOW_SHAPE
    bad, new = M.overflow_then_clean(N, S, M.seed_of(W, N, S))
    exp = oracle.eqcounts_ut(new)
    monkeypatch.setenv("D2G_BS_TAGBITS", "0")
    g = Group(d2g, torch, W, N, S)
    staged = [g.stage(bad), g.stage(new)]
    outs = g.slabs()
    torch.cuda.synchronize()
    g.feed(staged[0], 0)
    g.step(None, outs)
    for r in range(W):
        with pytest.raises(d2g.D2GError):
            g.engs[r].status(g.sp[r])
        with pytest.raises(d2g.D2GError):
            g.engs[r].operand().status(g.sp[r])
    monkeypatch.delenv("D2G_BS_TAGBITS")
    for c in g.ctxs:
        c.reload_tuning()
    g.feed(staged[1], 1)
    g.step(None, outs)
    got = g.clones(outs)
    torch.cuda.synchronize()
    for r in range(W):
        np.testing.assert_array_equal(outs[r].words(got[r]), g.expected(exp, r), err_msg=f"rank {r}")
    g.assert_clean()
    g.close()


# ---------------------------------------------------------------- 5. d2g_bcast_sigs with three loopback contexts
def test_bcast_sigs_to_three_loopback_contexts(d2g, oracle, torch):
    """every returned pointer holds the matrix bit for bit; one step whose row pointers are slices of those buffers, against the oracle"""
    W, N, S = 3, 517, 96
    m = M.sequence(N, S, 1, M.seed_of(W, N, S), M.PLANTED_KINDS)[0]
    bits = m.view(np.uint64)
    g = Group(d2g, torch, W, N, S)
    ptrs = d2g.bcast_sigs(g.ctxs, g.comms, bits)
    assert len(set(ptrs)) == W and all(ptrs)
    for r in range(W):
        back = np.empty((N, S), np.uint64)
        g.ctxs[r].d2h(back, ptrs[r])
        np.testing.assert_array_equal(back, bits, err_msg=f"context {r}")
    outs = g.slabs()
    torch.cuda.synchronize()
    for r in range(W):
        with torch.cuda.stream(g.streams[r]):
            if r % 2:
                keep_busy(torch)
    d2g.allpairs_step_all(g.engs, [ptrs[r] + g.held[r][0] * S * 8 for r in range(W)], None, [o.ptr for o in outs], g.sp)
    got = g.clones(outs)
    torch.cuda.synchronize()
    exp = oracle.eqcounts_ut(m)
    for r in range(W):
        np.testing.assert_array_equal(outs[r].words(got[r]), g.expected(exp, r), err_msg=f"rank {r}")
    g.assert_clean()
    for r in range(W):
        g.ctxs[r].free(ptrs[r])
    g.close()


# ---------------------------------------------------------------- 6. per-rank entry points on a multi-rank loopback group
@pytest.mark.parametrize("sparse", [False, True])
def test_per_rank_entry_points_are_refused_on_a_loopback_group(d2g, oracle, torch, monkeypatch, sparse):
    """d2g_allpairs_step_eqcount_dev, _prepare_dev and _enqueue_lut_dev on ONE engine of a two-rank loopback group cannot meet their
    peer's transfers.  They return D2G_ERR_INVALID with a message BEFORE anything is enqueued: no hang, the output and its guard words
    unchanged -- also where the sparse path is on and a step's first act would be the fill of its announced output -- nothing pending in
    the group.  The next d2g_allpairs_step_all of the group, on other matrices, is exact."""
    if sparse:
        monkeypatch.setenv("D2G_BS_SPARSE_MIN_N", "1")
    W, N, S = 2, 263, 1000
    assert (W, N, S) in M.STREAM_SHAPES
    mats = M.sequence(N, S, 3, M.seed_of(W, N, S), M.PLANTED_KINDS)
    exps = [oracle.eqcounts_ut(m) for m in mats]
    g = Group(d2g, torch, W, N, S)
    lut, luts = _tables(d2g, torch, S, W)["plus7"]
    staged = [g.stage(m) for m in mats]
    outs, spare = g.slabs(), g.slabs()
    torch.cuda.synchronize()
    g.feed(staged[0], 0)
    g.step(None, outs)
    got0 = g.clones(outs)
    INVALID = -1                                                      # D2G_ERR_INVALID (include/d2g.h)
    for r, call in ((0, lambda e, r: e.step_eqcount_dev(g.rows[r].data_ptr(), spare[r].ptr, g.sp[r])),
                    (1, lambda e, r: e.prepare_dev(g.rows[r].data_ptr(), g.sp[r])),
                    (0, lambda e, r: e.enqueue_lut_dev(g.rows[r].data_ptr(), luts[r].data_ptr(), spare[r].ptr, g.sp[r], input_ready=False)),
                    (1, lambda e, r: e.step_lut_dev(g.rows[r].data_ptr(), luts[r].data_ptr(), spare[r].ptr, g.sp[r]))):
        with pytest.raises(d2g.D2GError, match="loopback group") as err:
            call(g.engs[r], r)
        assert err.value.status == INVALID
    with pytest.raises(d2g.D2GError, match="loopback group"):        # the whole group, but one rank twice
        d2g.allpairs_step_all([g.engs[0], g.engs[0]], [g.rows[0].data_ptr()] * 2, None, [spare[0].ptr] * 2, [g.sp[0]] * 2)
    g.feed(staged[1], 1)
    g.step(None, outs)
    got1 = g.clones(outs)
    g.feed(staged[2], 2)
    g.step(luts, outs)
    got2 = g.clones(outs)
    torch.cuda.synchronize()
    for r in range(W):
        spare[r].assert_untouched()
        np.testing.assert_array_equal(outs[r].words(got0[r]), g.expected(exps[0], r), err_msg=f"before, rank {r}")
        np.testing.assert_array_equal(outs[r].words(got1[r]), g.expected(exps[1], r), err_msg=f"after (counts), rank {r}")
        np.testing.assert_array_equal(outs[r].words(got2[r]), g.expected(exps[2], r, lut), err_msg=f"after (table), rank {r}")
    g.assert_clean()
    g.close()
