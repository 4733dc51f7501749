"""The device-resident sketch entry points that the benchmark times -- d2g_oph_plan_create + d2g_oph_sketch_dev, d2g_oph_count_dev
and d2g_bmh_sketch_dev -- against the expected values of sketch_dev_cases.py, which no part of the library computed.  Everything is
compared bit for bit (BagMinHash registers as uint64).

What these forms do not share with the host-pointer and sketcher forms, and what is aimed at it here:
    launch tables    the plan's device copy of them, re-used over other packed buffers and other base pointers (b, d)
    stream           the caller's, null or not; K1 and the count pass do not synchronise.  Every case runs on the null stream and on a
                     torch side stream.  On the side stream the library is called while the stream is still busy and the packed buffer
                     still holds ANOTHER input: the copy of the right input is queued on that stream just before the call, and the
                     outputs are cloned on it just after.  Work that the library put on another stream without a fence reads the
                     wrong input or is cloned too early (c)
    K3 work state    the context's own, grow-only and shared by every call; the sub-batch pipeline's second stream (d, e)
    layout           64-byte-aligned slots in a buffer of random bytes, runs that start anywhere, overlap, or are missing (a, variants)

Every output has guard words behind it and starts as a pattern that no result contains; the guard words must come back untouched."""
import numpy as np
import pytest

import exact_ref as X
import oph_kmers_ref as R
import oph_mincount_ref as Q
import sketch_dev_cases as V
from gpu_ballast import keep_busy

pytestmark = pytest.mark.gpu

GUARD = 64                                                             # 8-byte words behind every output
REG_FILL = 0xABABABABABABABAB                                          # registers and counts start as 0xAB bytes
NAN_FILL = 0x7FF8DEADBEEF0001                                          # signatures and weights as a NaN no arithmetic produces
INF_BITS = np.float64(np.inf).view(np.uint64)
INVALID, UNSUPPORTED = -1, -5                                          # D2G_ERR_INVALID, D2G_ERR_UNSUPPORTED (include/d2g.h)


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


@pytest.fixture(params=["null", "side"])
def side(request, torch):
    """None: the null stream; else a torch.cuda.Stream()"""
    return torch.cuda.Stream() if request.param == "side" else None


class Out:
    """a device output of nbytes with GUARD words behind it, every word of both = fill"""

    def __init__(self, torch, nbytes, fill):
        assert nbytes % 8 == 0
        self.nw, self.fill = nbytes // 8, np.uint64(fill)
        self.t = torch.full((self.nw + GUARD,), int(np.uint64(fill).view(np.int64)), dtype=torch.int64, device="cuda")

    @property
    def ptr(self):
        return self.t.data_ptr()

    def words(self, t=None):
        """all words on the host (of a clone of the buffer, if one is given); the guard words must be as they were"""
        host = (self.t if t is None else t).cpu().numpy().view(np.uint64)
        assert (host[self.nw:] == self.fill).all(), "the guard words behind an output were written"
        return host[:self.nw]

    def read(self, dtype, shape, t=None):
        return self.words(t).view(dtype).reshape(shape)

    def assert_untouched(self):
        assert (self.words() == self.fill).all(), "a refused or empty call wrote to its output"


def device_bytes(torch, arr):
    return torch.from_numpy(np.array(arr, np.uint8)).cuda()


def on_stream(torch, side, A, B, call):
    """call(packed_ptr, stream) with input A in the device buffer; -> what `call` returns (clones of its outputs, made on the same stream).
    Null stream: upload, call.  Side stream: input B is sketched first; then, the stream kept busy, the buffer is overwritten with A
    on that stream, the library is called at once and the outputs are cloned on that stream; one synchronisation at the end."""
    packed = torch.empty_like(A)
    if side is None:
        packed.copy_(A)
        got = call(packed.data_ptr(), None)
        torch.cuda.synchronize()
        return got
    torch.cuda.synchronize()                                           # the fills of the outputs (null stream) are done
    with torch.cuda.stream(side):
        packed.copy_(B)
        call(packed.data_ptr(), side.cuda_stream)
        keep_busy(torch)
        packed.copy_(A)
        got = call(packed.data_ptr(), side.cuda_stream)
    side.synchronize()
    return got


def run_k1(gpu_ctx, torch, side, plan, n, A, B, S, canon, xormask, base=0, regs=None):
    """K1, then the count pass on the same stream with no host synchronisation between the two -> (registers [n][m], counts [n][m])"""
    m = R.oph_m(S)
    regs = regs or Out(torch, n * m * 8, REG_FILL)
    cnts = Out(torch, n * m * 4, REG_FILL)

    def call(ptr, stream):
        gpu_ctx.oph_sketch_dev(plan, ptr + base, S, regs.ptr, canon=canon, xormask=xormask, stream=stream)
        gpu_ctx.oph_count_dev(plan, ptr + base, S, regs.ptr, cnts.ptr, canon=canon, xormask=xormask, stream=stream)
        return regs.t.clone(), cnts.t.clone()
    r, c = on_stream(torch, side, A, B, call)
    return regs.read(np.uint64, (n, m), r), cnts.read(np.uint32, (n, m), c)


def run_k3(gpu_ctx, torch, side, plan, n, A, B, S, thr, canon=True, xormask=0, base=0):
    """-> (registers float64 [n][S], total weights [n])"""
    sig, tw = Out(torch, n * S * 8, NAN_FILL), Out(torch, n * 8, NAN_FILL)

    def call(ptr, stream):
        gpu_ctx.bmh_sketch_dev(plan, ptr + base, S, sig.ptr, tw.ptr, canon=canon, xormask=xormask, count_threshold=thr, stream=stream)
        return sig.t.clone(), tw.t.clone()
    s, t = on_stream(torch, side, A, B, call)
    return sig.read(np.float64, (n, S), s), tw.read(np.float64, (n,), t)


def assert_k1(got, exp, what):
    np.testing.assert_array_equal(got[0], exp[0], err_msg=what + ": registers")
    np.testing.assert_array_equal(got[1], exp[1], err_msg=what + ": counts")


def assert_k3(got, exp, what):
    np.testing.assert_array_equal(got[1], exp[1], err_msg=what + ": total weights")
    np.testing.assert_array_equal(got[0].view(np.uint64), exp[0].view(np.uint64), err_msg=what + ": registers")


class AsSeqPack:
    """a layout where a Sketcher's run* and Context.kmer_filter want a SeqPack"""

    def __init__(self, lay, k):
        self.lay, self.k = lay, k

    def arrays(self):
        return (np.array(self.lay.packed),) + tuple(np.array(a) for a in self.lay.tables())


def assert_host_forms(gpu_ctx, lay, k, S, canon, xormask, exp, what):
    """the host-pointer forms of K1 over the layout's own arrays -- the one-shots d2g_oph_sketch and d2g_oph_sketch_counts, and
    d2g_sketcher_run and d2g_sketcher_run_counts on one sketcher -- against the expected (registers, counts), bit for bit"""
    sp = AsSeqPack(lay, k)
    sk = gpu_ctx.sketcher()
    got = [("d2g_oph_sketch", gpu_ctx.oph_sketch(lay.packed, *lay.tables(), k, S, canon=canon, xormask=xormask), None),
           ("d2g_oph_sketch_counts",) + gpu_ctx.oph_sketch_counts(lay.packed, *lay.tables(), k, S, canon=canon, xormask=xormask),
           ("d2g_sketcher_run", sk.run(sp, S, canon, xormask), None),
           ("d2g_sketcher_run_counts",) + sk.run_counts(sp, S, canon, xormask)]
    sk.close()
    for form, regs, cnts in got:
        np.testing.assert_array_equal(regs, exp[0], err_msg=f"{what}: {form}: registers")
        if cnts is not None:
            np.testing.assert_array_equal(cnts, exp[1], err_msg=f"{what}: {form}: counts")


class AsBatch:
    """a layout's distinct keys and counts where exact_ref wants a k3_seam_cases.Batch"""

    def __init__(self, lay, k, canon, xormask):
        self.kc = lay.key_counts(k, canon, xormask)

    def counts(self):
        return self.kc


def mincount_expected(lay, k, canon, xormask, S, c):
    """-> (registers [n][m], counts [n][m]) over the k-mers seen at least c times: oph_mincount_ref.closed_form per genome"""
    m = R.oph_m(S)
    regs, cnts = np.empty((lay.n, m), np.uint64), np.empty((lay.n, m), np.uint32)
    for g, (keys, counts, _) in enumerate(lay.key_counts(k, canon, xormask)):
        regs[g], cnts[g] = Q.closed_form(keys, counts, m, c)
    return regs, cnts


def run_mincount_dev(gpu_ctx, torch, plan, n, p, S, c, canon, xormask):
    """plan + d2g_oph_sketch_mincount_dev, then d2g_oph_count_dev over its registers -> (registers [n][m], counts [n][m])"""
    m = R.oph_m(S)
    regs, cnts = Out(torch, n * m * 8, REG_FILL), Out(torch, n * m * 4, REG_FILL)
    torch.cuda.synchronize()
    gpu_ctx.oph_sketch_mincount_dev(plan, p, S, c, regs.ptr, canon=canon, xormask=xormask)
    gpu_ctx.oph_count_dev(plan, p, S, regs.ptr, cnts.ptr, canon=canon, xormask=xormask)
    torch.cuda.synchronize()
    return regs.read(np.uint64, (n, m)), cnts.read(np.uint32, (n, m))


def run_sets_dev(gpu_ctx, torch, plan, n, p, cap, canon, xormask, counts=True):
    """plan + d2g_kmer_sets_dev into guarded device arrays of cap entries -> (keys, counts or None, set_off [n+1], cards [n][2])"""
    room = (max(cap, 1) + 1) // 2 * 2
    keys, cnts = Out(torch, room * 8, REG_FILL), Out(torch, room * 4, REG_FILL)
    off, cards = Out(torch, (n + 1) * 8, REG_FILL), Out(torch, max(n, 1) * 16, REG_FILL)
    torch.cuda.synchronize()
    gpu_ctx.kmer_sets_dev(plan, p, keys.ptr, cnts.ptr if counts else None, cap, off.ptr, cards.ptr, canon=canon, xormask=xormask)
    torch.cuda.synchronize()
    o = off.read(np.uint64, (n + 1,))
    total = int(o[n])
    if not counts:
        cnts.assert_untouched()
    return (keys.read(np.uint64, (room,))[:total], cnts.read(np.uint32, (2 * (room // 2),))[:total] if counts else None, o,
            cards.read(np.uint64, (max(n, 1), 2))[:n])


def assert_sets(got, exp, counts, what):
    keys, cnts, off, cards = got
    np.testing.assert_array_equal(off, exp[2], err_msg=what + ": set_off")
    np.testing.assert_array_equal(cards, exp[3], err_msg=what + ": cards")
    np.testing.assert_array_equal(keys, exp[0], err_msg=what + ": keys")
    if counts:
        np.testing.assert_array_equal(cnts, exp[1], err_msg=what + ": counts")
    else:
        assert cnts is None, what


# ---------------------------------------------------------------- a. K1 at the plan's seams
@pytest.mark.parametrize("xormask", [0, V.SEEDED], ids=["mask0", "seeded"])
@pytest.mark.parametrize("canon", [True, False], ids=["canon", "fwd"])
@pytest.mark.parametrize("k", [31, 32])
def test_k1_at_the_plans_seams(gpu_ctx, torch, side, k, canon, xormask):
    """genomes of 1, 63, 64, 65, 65 536, 65 537 and 131 073 k-mers (a lane chunk, a workgroup's share, three workgroups that merge in
    HBM) at m = 1000, 1024, 16 384 (the last in LDS), 16 386 (the first in HBM and no power of two: k1_oph_kernel<false, false>) and
    20 000; the count pass leaves LDS above m = 10 922.  At the two HBM sizes the host-pointer forms take the same input"""
    lay, other = V.seams(k), V.seams(k, 3101)
    A, B = device_bytes(torch, lay.packed), device_bytes(torch, other.packed)
    plan = gpu_ctx.oph_plan(*lay.tables(), k)
    assert plan.nkmers == sum(V.SEAM_KMERS) and plan.nbases == int(lay.run_len.sum())
    for S in V.SEAM_SIZES:
        exp = lay.oph(k, canon, xormask, S)
        got = run_k1(gpu_ctx, torch, side, plan, lay.n, A, B, S, canon, xormask)
        assert_k1(got, exp, f"{lay} S {S}")
        if S > 16384 and side is None:
            assert_host_forms(gpu_ctx, lay, k, S, canon, xormask, exp, f"{lay} S {S}")
    plan.close()


@pytest.mark.parametrize("which", V.VARIANTS)
def test_k1_through_other_tables_over_the_same_bytes(gpu_ctx, torch, side, which):
    """runs that start at any base, two runs per genome across a workgroup's end, overlapping genomes, genomes without a run, runs in
    descending stream order"""
    k = 31
    lay, other = V.variant(which, k), V.variant(which, k, 3201)
    A, B = device_bytes(torch, lay.packed), device_bytes(torch, other.packed)
    plan = gpu_ctx.oph_plan(*lay.tables(), k)
    for S, canon, xormask in ((1000, True, V.SEEDED), (16385, False, 0)):
        got = run_k1(gpu_ctx, torch, side, plan, lay.n, A, B, S, canon, xormask)
        assert_k1(got, lay.oph(k, canon, xormask, S), f"{lay} S {S}")
    plan.close()


FRONT_DOORS = [(lambda w=w: V.variant(w, 31), 31, V.SEEDED) for w in V.VARIANTS] + [
    (V.multiset_slots, V.K3_K, 0), (lambda: V.k3_reuse_step(1), V.K3_K, 0), (lambda: V.nothing(3), V.K3_K, 0)]


@pytest.mark.parametrize("case", FRONT_DOORS, ids=list(V.VARIANTS) + ["multiset_slots", "one_and_none", "nothing3"])
def test_every_front_door_gives_the_same(gpu_ctx, torch, case):
    """one layout through every way in.  K1: the one-shots, a sketcher and plan + *_dev give the layout's own expected registers and
    counts, so the same bits as each other, at S = 64 and S = 1000.  The filter: d2g_kmer_filter_create and plan +
    d2g_kmer_filter_create_dev over the same runs hold the same set -- the occurrences and distinct k-mers that the layout's bases
    hold, every one of its k-mers and none of 64 that it does not hold.  At the same sizes the registers over the k-mers seen twice
    (with and without counts) and BagMinHash; once per layout the distinct counts and the exact sets (with and without counts):
    the one-shot, a sketcher and, where there is one, plan + *_dev, each against the restatement of oph_mincount_ref, Layout.bmh
    and exact_ref, so bit for bit like each other"""
    make, k, xormask = case
    lay, canon = make(), True
    A = device_bytes(torch, lay.packed)
    plan = gpu_ctx.oph_plan(*lay.tables(), k)
    sp, sk = AsSeqPack(lay, k), gpu_ctx.sketcher()
    for S in (64, 1000):
        exp = lay.oph(k, canon, xormask, S)
        assert_k1(run_k1(gpu_ctx, torch, None, plan, lay.n, A, None, S, canon, xormask), exp, f"{lay} S {S}: plan + dev")
        assert_host_forms(gpu_ctx, lay, k, S, canon, xormask, exp, f"{lay} S {S}")
        exp = mincount_expected(lay, k, canon, xormask, S, 2)
        assert_k1(run_mincount_dev(gpu_ctx, torch, plan, lay.n, A.data_ptr(), S, 2, canon, xormask), exp, f"{lay} S {S}: mincount, plan + dev")
        for form, f in (("d2g_oph_sketch_mincount", gpu_ctx.oph_sketch_mincount_seqpack), ("d2g_sketcher_run_mincount", sk.run_mincount)):
            assert_k1(f(sp, S, 2, canon, xormask, counts=True), exp, f"{lay} S {S}: {form}")
            np.testing.assert_array_equal(f(sp, S, 2, canon, xormask), exp[0], err_msg=f"{lay} S {S}: {form} without counts")
        exp = lay.bmh(k, canon, xormask, S, 0.0)
        assert_k3(run_k3(gpu_ctx, torch, None, plan, lay.n, A, None, S, 0.0, canon=canon, xormask=xormask), exp, f"{lay} S {S}: bmh, plan + dev")
        assert_k3(gpu_ctx.bmh_sketch_seqpack(sp, S, canon, xormask), exp, f"{lay} S {S}: d2g_bmh_sketch")
        assert_k3(sk.run_bmh(sp, S, canon, xormask), exp, f"{lay} S {S}: d2g_sketcher_run_bmh")
    exp = X.flat(X.exact_sets(AsBatch(lay, k, canon, xormask)))
    for form, got in (("d2g_kmer_distinct", gpu_ctx.kmer_distinct_seqpack(sp, canon, xormask)), ("d2g_sketcher_run_distinct", sk.run_distinct(sp, canon, xormask))):
        np.testing.assert_array_equal(got, exp[3][:, 0], err_msg=f"{lay}: {form}")
    for counts in (True, False):
        assert_sets(gpu_ctx.kmer_sets_seqpack(sp, canon, xormask, counts=counts), exp, counts, f"{lay}: d2g_kmer_sets")
        assert_sets(sk.run_sets(sp, canon, xormask, counts=counts), exp, counts, f"{lay}: d2g_sketcher_run_sets")
        assert_sets(run_sets_dev(gpu_ctx, torch, plan, lay.n, A.data_ptr(), sum(lay.nkmers(k)), canon, xormask, counts), exp, counts,
                    f"{lay}: plan + d2g_kmer_sets_dev")
    sk.close()
    kmers = np.concatenate([V.kmers_np(lay.run_codes(r), k, canon) for r in range(lay.nrun)] + [np.zeros(0, np.uint64)])
    held = np.unique(kmers)
    absent = np.random.default_rng(3800).integers(0, 1 << (2 * k), 80, dtype=np.uint64)
    absent = absent[~np.isin(absent, held)][:64]
    assert absent.size == 64
    ask = np.concatenate([kmers, absent])
    filters = [gpu_ctx.kmer_filter(AsSeqPack(lay, k), canon), gpu_ctx.kmer_filter_dev(plan, A.data_ptr(), canon)]
    for f, form in zip(filters, ("d2g_kmer_filter_create", "plan + d2g_kmer_filter_create_dev")):
        assert f.info()[:2] == (kmers.size, held.size), f"{lay}: {form}"
        np.testing.assert_array_equal(f.contains(ask), np.arange(ask.size) < kmers.size, err_msg=f"{lay}: {form}")
        f.close()
    plan.close()


# ---------------------------------------------------------------- b. one plan, many inputs
def test_k1_plan_reuse(gpu_ctx, torch, side):
    """one plan of three slots over three packed buffers and over the base pointers packed + b0 * slot_bytes, with S, canon and the
    mask changing from call to call; then two inputs, one after the other, into the SAME output: the second result holds nothing of
    the first (on the side stream every call is such a second call: input B went into the same output before)"""
    k = 31
    lays = [V.reuse_buffer(i) for i in range(3)]
    dev = [device_bytes(torch, l.packed) for l in lays]
    slot = lays[0].slot_bytes
    plan = gpu_ctx.oph_plan(*lays[0].head(3), k)
    calls = [(0, 0, 1000, True, 0), (1, 0, 1024, False, V.SEEDED), (2, 3, 1000, True, V.SEEDED), (0, 3, 16385, False, 0),
             (1, 3, 1024, True, 0), (2, 0, 1000, True, 0)]
    for i, b0, S, canon, xormask in calls:
        lays[i].head(3, b0)                                             # in bounds at that base pointer
        got = run_k1(gpu_ctx, torch, side, plan, 3, dev[i], dev[(i + 1) % 3], S, canon, xormask, base=b0 * slot)
        exp = lays[i].oph(k, canon, xormask, S)
        assert_k1(got, (exp[0][b0:b0 + 3], exp[1][b0:b0 + 3]), f"{lays[i]} slots {b0}.. S {S} canon {canon}")
    S = 1000
    regs = Out(torch, 3 * R.oph_m(S) * 8, REG_FILL)
    first = run_k1(gpu_ctx, torch, side, plan, 3, dev[1], dev[2], S, True, 0, regs=regs)
    second = run_k1(gpu_ctx, torch, side, plan, 3, dev[2], dev[0], S, True, 0, base=3 * slot, regs=regs)
    e1, e2 = lays[1].oph(k, True, 0, S), lays[2].oph(k, True, 0, S)
    assert_k1(first, (e1[0][:3], e1[1][:3]), "first call into the shared output")
    assert_k1(second, (e2[0][3:], e2[1][3:]), "second call into the shared output")
    assert (np.minimum(e1[0][:3], e2[0][3:]) != e2[0][3:]).any()         # minima kept from the first call would show
    plan.close()


# ---------------------------------------------------------------- d. K3 in the benchmark's layout
@pytest.mark.parametrize("thr", [0.0, 1.0])
@pytest.mark.parametrize("S", [64, 1000, 2048])
def test_k3_in_the_benchmarks_layout(gpu_ctx, torch, side, S, thr):
    """4 genomes per call at k = 21, two batches through one plan by pointer offset.  Threshold 1 leaves one element (of count 2) in
    one genome of the second batch and nothing anywhere else"""
    lay, other = V.multiset_slots(), V.multiset_slots(3401)
    A, B = device_bytes(torch, lay.packed), device_bytes(torch, other.packed)
    plan = gpu_ctx.oph_plan(*lay.head(4), V.K3_K)
    esig, etw = lay.bmh(V.K3_K, True, 0, S, thr)
    for b0 in (0, 1):
        lay.head(4, b0)
        got = run_k3(gpu_ctx, torch, side, plan, 4, A, B, S, thr, base=b0 * lay.slot_bytes)
        assert_k3(got, (esig[b0:b0 + 4], etw[b0:b0 + 4]), f"{lay} slots {b0}.. S {S} threshold {thr}")
    plan.close()


@pytest.mark.parametrize("which", V.VARIANTS)
def test_k3_through_other_tables_over_the_same_bytes(gpu_ctx, torch, side, which):
    """`overlap`: the 2980 k-mers that genome 3's two runs share have count 2 and are all that a threshold of 1 keeps"""
    k = V.K3_K
    lay, other = V.variant(which, k), V.variant(which, k, 3201)
    A, B = device_bytes(torch, lay.packed), device_bytes(torch, other.packed)
    plan = gpu_ctx.oph_plan(*lay.tables(), k)
    for S, thr, canon, xormask in ((64, 0.0, True, 0), (64, 1.0, True, 0), (255, 0.0, False, V.SEEDED)):
        got = run_k3(gpu_ctx, torch, side, plan, lay.n, A, B, S, thr, canon=canon, xormask=xormask)
        assert_k3(got, lay.bmh(k, canon, xormask, S, thr), f"{lay} S {S} threshold {thr} canon {canon}")
    plan.close()


def test_k3_work_state_is_reused_by_every_call(gpu_ctx, torch):
    """the context's K3 work state grows with the first batch and serves smaller and other ones after it; a sketcher's own state in
    between; the first batch once more gives the bits it gave before"""
    k = V.K3_K
    steps = [(V.k3_reuse_step(0), 256), (V.k3_reuse_step(1), 64), (V.k3_reuse_step(2), 1000)]

    def run(lay, S):
        plan = gpu_ctx.oph_plan(*lay.tables(), k)
        got = run_k3(gpu_ctx, torch, None, plan, lay.n, device_bytes(torch, lay.packed), None, S, 0.0)
        plan.close()
        assert_k3(got, lay.bmh(k, True, 0, S, 0.0), f"{lay} S {S}")
        return got
    first = run(*steps[0])
    sig, tw = run(*steps[1])
    assert tw[1] == 0.0 and (sig[1].view(np.uint64) == INF_BITS).all() and np.isfinite(sig[0]).all()
    run(*steps[2])
    sk = gpu_ctx.sketcher()
    lay = steps[2][0]
    assert_k3(sk.run_bmh(AsSeqPack(lay, k), 64), lay.bmh(k, True, 0, 64, 0.0), "the sketcher's own state")
    sk.close()
    again = run(*steps[0])
    assert np.array_equal(again[0].view(np.uint64), first[0].view(np.uint64)) and np.array_equal(again[1], first[1])


# ---------------------------------------------------------------- e. the sub-batch pipeline on the caller's stream
@pytest.mark.parametrize("light", [True, False], ids=["light", "one_kmer_short_of_light"])
@pytest.mark.parametrize("subbatch", [2, 3])
def test_k3_subbatch_pipeline_on_the_callers_stream(gpu_ctx, torch, side, monkeypatch, subbatch, light):
    """D2G_K3_SUBBATCH cuts a batch into genome ranges whose counting passes run on the library's second stream, fenced against the
    caller's by events.  That form runs only for a batch on the generic path (the default), not split, of n >= 2 genomes, whose first
    pass is light.  The smallest batch of three equal genomes that is light, at S = 64 and k = 21:
        K3Run::sketch stays light unless  sum_g gk min(1, guess_g) > (sum_g gk) / 8,  guess_g = 1.25 (S / gk) (ln S + 0.58 + 8)
        equal genomes:  min(1, guess) <= 1/8  <=>  gk >= 10 S (ln S + 8.58) = 640 * 12.7389 = 8152.9
    so gk = 8153 k-mers, runs of 8173 bases (8 buckets of ~1019 keys per genome: far below the 5600 at which buckets are split).
    With one k-mer fewer per genome the batch is heavy and bucketed in one range: the other side of the seam"""
    monkeypatch.setenv("D2G_K3_SUBBATCH", str(subbatch))
    assert gpu_ctx.tuning().get("D2G_K3_SUBBATCH") == str(subbatch)
    k, S = V.K3_K, 64
    lay, other = V.pipeline_batch(light), V.pipeline_batch(light, 3601)
    assert lay.nkmers(k) == [V.light_min_kmers(S) - (0 if light else 1)] * 3
    A, B = device_bytes(torch, lay.packed), device_bytes(torch, other.packed)
    plan = gpu_ctx.oph_plan(*lay.tables(), k)
    got = run_k3(gpu_ctx, torch, side, plan, 3, A, B, S, 0.0)
    assert_k3(got, lay.bmh(k, True, 0, S, 0.0), f"{lay} SUBBATCH {subbatch}")
    plan.close()


# ---------------------------------------------------------------- f. empty shapes
def test_a_plan_without_genomes_writes_nothing(gpu_ctx, torch, side):
    lay = V.nothing(0)
    packed = device_bytes(torch, lay.packed)
    plan = gpu_ctx.oph_plan(*lay.tables(), 31)
    assert plan.nkmers == 0 and plan.nbases == 0
    regs, cnts = Out(torch, 128, REG_FILL), Out(torch, 128, REG_FILL)
    sig, tw = Out(torch, 128, NAN_FILL), Out(torch, 128, NAN_FILL)
    stream = side.cuda_stream if side is not None else None
    torch.cuda.synchronize()
    gpu_ctx.oph_sketch_dev(plan, packed.data_ptr(), 1000, regs.ptr, stream=stream)
    gpu_ctx.oph_count_dev(plan, packed.data_ptr(), 1000, regs.ptr, cnts.ptr, stream=stream)
    gpu_ctx.bmh_sketch_dev(plan, packed.data_ptr(), 64, sig.ptr, tw.ptr, stream=stream)
    torch.cuda.synchronize()
    for o in (regs, cnts, sig, tw):
        o.assert_untouched()
    plan.close()


def test_genomes_without_a_run(gpu_ctx, torch, side):
    """n = 3 and no workgroup: empty registers -- K1 does not even look at the packed pointer --, zero counts, +inf and weight 0"""
    lay = V.nothing(3)
    packed = device_bytes(torch, lay.packed)
    plan = gpu_ctx.oph_plan(*lay.tables(), 21)
    S = 1000
    regs, cnts = Out(torch, 3 * S * 8, REG_FILL), Out(torch, 3 * S * 4, REG_FILL)
    sig, tw = Out(torch, 3 * 64 * 8, NAN_FILL), Out(torch, 3 * 8, NAN_FILL)
    stream = side.cuda_stream if side is not None else None
    torch.cuda.synchronize()
    gpu_ctx.oph_sketch_dev(plan, None, S, regs.ptr, stream=stream)
    gpu_ctx.oph_count_dev(plan, None, S, regs.ptr, cnts.ptr, stream=stream)
    gpu_ctx.bmh_sketch_dev(plan, packed.data_ptr(), 64, sig.ptr, tw.ptr, stream=stream)
    torch.cuda.synchronize()
    assert (regs.words() == np.uint64(R.M64)).all() and not cnts.words().any()
    assert (sig.words() == INF_BITS).all() and not tw.read(np.float64, (3,)).any()
    plan.close()


# ---------------------------------------------------------------- g. refusals
def refused(d2g, status, call, *args, **kw):
    with pytest.raises(d2g.D2GError) as e:
        call(*args, **kw)
    assert e.value.status == status, str(e.value)


def test_dev_calls_refuse_bad_arguments_and_write_nothing(gpu_ctx, d2g, torch):
    """every plan form against a plan of another context, a packed pointer off by 1 or 2 and a null packed pointer under a plan with
    blocks: D2G_ERR_INVALID and nothing written (the forms that always refused a null stream first); then the wrong sizes and null
    outputs; then every form with the same arguments put right"""
    k, S, canon = 21, 64, True
    lay = V.multiset_slots()
    packed = device_bytes(torch, lay.packed)
    p = packed.data_ptr()
    plan = gpu_ctx.oph_plan(*lay.head(4), k)
    m = R.oph_m(S)
    kc = lay.key_counts(k, canon, 0)[:4]
    cap = sum(lay.nkmers(k)[:4])
    room = (cap + 1) // 2 * 2
    regs, cnts = Out(torch, 4 * m * 8, REG_FILL), Out(torch, 4 * m * 4, REG_FILL)
    sig, tw = Out(torch, 4 * S * 8, NAN_FILL), Out(torch, 4 * 8, NAN_FILL)
    keys, kcnt = Out(torch, room * 8, REG_FILL), Out(torch, room * 4, REG_FILL)
    off, cards = Out(torch, 5 * 8, REG_FILL), Out(torch, 4 * 16, REG_FILL)
    db = kc[0][0][:S].reshape(1, S)                                    # a database of one reference: 64 masked k-mers of genome 0
    screen = gpu_ctx.screen(db, k, canon=canon, xormask=0, nrows=1)
    rows = [0, 0, 0, 0]
    torch.cuda.synchronize()
    other_ctx = d2g.Context(0)
    foreign = other_ctx.oph_plan(*lay.head(4), k)
    forms = [                                                          # (call, arguments after (plan, packed)); K3's two last
        (gpu_ctx.oph_sketch_dev, (S, regs.ptr)), (gpu_ctx.oph_count_dev, (S, regs.ptr, cnts.ptr)),
        (gpu_ctx.oph_sketch_mincount_dev, (S, 2, regs.ptr)), (gpu_ctx.kmer_filter_dev, ()), (screen.add_dev, (rows,)),
        (gpu_ctx.bmh_sketch_dev, (S, sig.ptr, tw.ptr)), (gpu_ctx.kmer_sets_dev, (keys.ptr, kcnt.ptr, cap, off.ptr, cards.ptr)),
    ]
    for i, (call, args) in enumerate(forms):
        for wrong in ((foreign, p), (plan, p + 1 + i % 2), (plan, None)):
            refused(d2g, INVALID, call, *wrong, *args)
    bad = [
        (gpu_ctx.oph_sketch_dev, (plan, p, 0, regs.ptr)), (gpu_ctx.oph_count_dev, (plan, p, 0, regs.ptr, cnts.ptr)),
        (gpu_ctx.bmh_sketch_dev, (plan, p, 0, sig.ptr, tw.ptr)), (gpu_ctx.bmh_sketch_dev, (plan, p, 1 << 24, sig.ptr, tw.ptr)),
        (gpu_ctx.oph_sketch_dev, (plan, p, 1 << 31, regs.ptr)),
        (gpu_ctx.oph_sketch_dev, (plan, p, S, None)), (gpu_ctx.oph_count_dev, (plan, p, S, None, cnts.ptr)),
        (gpu_ctx.oph_count_dev, (plan, p, S, regs.ptr, None)),
        (gpu_ctx.bmh_sketch_dev, (plan, p, S, None, tw.ptr)), (gpu_ctx.bmh_sketch_dev, (plan, p, S, sig.ptr, None)),
    ]
    for call, args in bad:
        refused(d2g, INVALID, call, *args)
    refused(d2g, INVALID, gpu_ctx.bmh_sketch_dev, plan, p, S, sig.ptr, tw.ptr, count_threshold=float("nan"))
    torch.cuda.synchronize()
    for o in (regs, cnts, sig, tw, keys, kcnt, off, cards):
        o.assert_untouched()
    assert screen.fed(0) == 0 and not screen.key_counts(0)[1].any()
    # the same arguments, put right, are served: the refusals above were of what was wrong with them
    gpu_ctx.bmh_sketch_dev(plan, p, S, sig.ptr, tw.ptr)
    torch.cuda.synchronize()
    assert_k3((sig.read(np.float64, (4, S)), tw.read(np.float64, (4,))), tuple(a[:4] for a in lay.bmh(k, True, 0, S, 0.0)), "after the refusals")
    gpu_ctx.oph_sketch_dev(plan, p, S, regs.ptr)
    gpu_ctx.oph_count_dev(plan, p, S, regs.ptr, cnts.ptr)
    torch.cuda.synchronize()
    assert_k1((regs.read(np.uint64, (4, m)), cnts.read(np.uint32, (4, m))), tuple(a[:4] for a in lay.oph(k, canon, 0, S)), "after the refusals")
    gpu_ctx.oph_sketch_mincount_dev(plan, p, S, 2, regs.ptr)
    np.testing.assert_array_equal(regs.read(np.uint64, (4, m)), mincount_expected(lay, k, canon, 0, S, 2)[0][:4], err_msg="after the refusals")
    gpu_ctx.kmer_sets_dev(plan, p, keys.ptr, kcnt.ptr, cap, off.ptr, cards.ptr)
    torch.cuda.synchronize()
    exp = X.flat([(ks, cs) for ks, cs, _ in kc])
    total = int(exp[2][4])
    assert_sets((keys.read(np.uint64, (room,))[:total], kcnt.read(np.uint32, (room,))[:total], off.read(np.uint64, (5,)),
                 cards.read(np.uint64, (4, 2))), exp, True, "after the refusals")
    f = gpu_ctx.kmer_filter_dev(plan, p, canon)
    assert f.info()[:2] == (cap, np.unique(np.concatenate([V.kmers_np(lay.run_codes(g), k, canon) for g in range(4)])).size)
    f.close()
    screen.add_dev(plan, p, rows)
    hits = sum(cs[np.isin(ks, db)].astype(np.int64).sum() for ks, cs, _ in kc)
    assert screen.fed(0) == cap and int(screen.key_counts(0)[1].sum()) == hits > 0
    screen.close()
    foreign.close()
    other_ctx.close()
    plan.close()


def test_plan_create_refuses_bad_tables(gpu_ctx, d2g):
    rs, rl = np.array([0, 400], np.uint64), np.array([100, 50], np.uint32)
    refused(d2g, UNSUPPORTED, gpu_ctx.oph_plan, rs, rl, [0, 1, 2], 33)
    refused(d2g, INVALID, gpu_ctx.oph_plan, rs, np.array([100, 30], np.uint32), [0, 1, 2], 31)     # a run shorter than k
    refused(d2g, INVALID, gpu_ctx.oph_plan, rs, rl, [0, 1, 1], 31)                                # genome_run_off[n] != nrun
    refused(d2g, INVALID, gpu_ctx.oph_plan, rs, rl, [0, 1, 3], 31)
    refused(d2g, INVALID, gpu_ctx.oph_plan, rs, rl, [0, 2, 1, 2], 31)                             # not monotone
    gpu_ctx.oph_plan(rs, rl, [0, 1, 2], 32).close()                                               # k = 32 and a run of k + 18 are fine
