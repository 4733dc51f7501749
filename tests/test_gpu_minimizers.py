"""Windowed minimizers on the GPU (K1w: the WIN mode of the shared walker, d2g_kmers.h + d2g_minq.h) against the model of
tests/minimizer_ref.py.  First the emitted multiset itself -- Sketcher.run_sets with counts is the exact (k-mer, number of window
positions) table of every genome -- at every seam of the decomposition; then every consumer once or twice against the UNCHANGED oracle
over the input rewritten as one k-base record per emission.  Every comparison is exact."""
import numpy as np
import pytest

import contain_ref as CR
import minimizer_ref as MR
import oph_kmers_ref as R
import oph_mincount_ref as Q
from dashing2_amd import synth

pytestmark = pytest.mark.gpu
INVALID, UNSUPPORTED = -1, -5                                          # D2G_ERR_INVALID, D2G_ERR_UNSUPPORTED (include/d2g.h)

# emissions of a run, E = len - w + 1: around a packed word's 16, a lane's chunk (64), two chunks, one 256-lane pass (16384) and one
# workgroup (65536)
SEAMS = (0, 1, 2, 63, 64, 65, 127, 128, 129, 16383, 16384, 16385, 65535, 65536, 65537)
KW = [(21, 22, True), (21, 36, False), (21, 37, True), (31, 94, True), (31, 95, False), (5, 7, True), (32, 33, False), (32, 100, True),
      (15, 1038, True)]


def _seq(seed, n):
    return synth.random_genome(seed, n).tobytes()


def _fa(seq, name="g"):
    return b">" + name.encode() + b"\n" + seq + b"\n"


def _pack(d2g, fastas, k):
    sp = d2g.SeqPack(k)
    for f in fastas:
        sp.add_fastx(f)
    return sp


def _check_sets(d2g, sk, fastas, k, w, canon):
    """run_sets of the windowed sketcher == the model's multiset, genome by genome; -> emissions per genome"""
    keys, counts, off, cards = sk.run_sets(_pack(d2g, fastas, k), canon=canon)
    total = []
    for g, fa in enumerate(fastas):
        em = MR.fasta_emissions(fa, k, w, canon, fast=True)
        ek, ec = MR.masked_counts(em)
        lo, hi = int(off[g]), int(off[g + 1])
        assert np.array_equal(keys[lo:hi], ek) and np.array_equal(counts[lo:hi], ec), (g, len(em), hi - lo, ek.size)
        assert cards[g].tolist() == [ek.size, len(em)]
        total.append(len(em))
    return total


@pytest.mark.parametrize("k,w,canon", KW, ids=[f"k{k}w{w}{'c' if c else 'f'}" for k, w, c in KW])
def test_emitted_multiset_at_every_seam(d2g, gpu_ctx, k, w, canon):
    """one genome per seam, each a single random run of E + w - 1 bases (E = 0: one base short of a window, still >= k: it stays in
    the stream and owns no chunk)"""
    fastas = [_fa(_seq(1000 + i, E + w - 1)) for i, E in enumerate(SEAMS)]
    sk = gpu_ctx.sketcher()
    sk.set_window(w)
    assert _check_sets(d2g, sk, fastas, k, w, canon) == list(SEAMS)
    sk.close()


def _kinds(k, w):
    q = w - k + 1
    n = 3000 + 2 * w
    out = {"polyA": b"A" * n, "AC": b"AC" * (n // 2)}
    for per in (q - 1, q, q + 1):
        if per >= 1:
            out[f"period{per - q:+d}"] = (_seq(per, per) * (n // per + 1))[:n]
    base = _seq(77, n)
    for gap in (w - 1, w, w + 1):
        b = bytearray(base)
        b[gap::gap + 1] = b"N" * len(b[gap::gap + 1])                  # an N after every `gap` bases: runs of gap bases
        out[f"N{gap - w:+d}"] = bytes(b)
    return out


@pytest.mark.parametrize("k,w,canon", [(21, 22, True), (21, 37, False), (31, 95, True), (5, 7, False), (32, 100, False), (15, 1038, True)],
                         ids=["k21w22", "k21w37", "k31w95", "k5w7", "k32w100", "k15w1038"])
def test_emitted_multiset_of_repetitive_and_broken_sequences(d2g, gpu_ctx, k, w, canon):
    """poly-A (the leaving minimum is replaced by its equal), (AC)n, a unit repeated with period q - 1, q, q + 1 (the minimum leaves once
    per period), an N every w - 1, w, w + 1 bases (runs without a window, with one, with two), all in ONE batch -- whose genome N-1
    has only runs shorter than w"""
    kinds = _kinds(k, w)
    names = sorted(kinds)
    sk = gpu_ctx.sketcher()
    sk.set_window(w)
    total = dict(zip(names, _check_sets(d2g, sk, [_fa(kinds[n], n) for n in names], k, w, canon)))
    assert total["N-1"] == 0 and total["N+0"] > 0 and total["N+1"] > total["N+0"] and total["polyA"] == len(kinds["polyA"]) - w + 1
    # the same genomes in one multi-record input: nothing spans records
    joined = b"".join(_fa(kinds[n], n) for n in names)
    assert _check_sets(d2g, sk, [joined], k, w, canon) == [sum(total.values())]
    sk.close()


# ---- every consumer against the oracle over the rewritten input ----------------------------------------------------------------------
def _genomes(w):
    g0 = _seq(500, 70000)                                              # more window positions than one workgroup walks
    g1 = bytearray(_seq(501, 4000))
    g1[700:709] = b"N" * 9
    g1[1500:1501] = b"N"
    g1[1500 + w - 1:1500 + w] = b"N"                                   # a run of w - 2 bases between two Ns
    rep = _seq(502, 1500)
    return [_fa(g0, "g0"), _fa(bytes(g1), "g1"), _fa(rep, "r0") + _fa(rep[200:900], "r1") + _fa(rep, "r2"),
            _fa(_seq(503, w - 1), "short") + _fa(_seq(504, w - 1), "short2"), b">empty\n\n"]


_MODEL = {}


def _model(k, w, canon):
    if (k, w, canon) not in _MODEL:
        gs = _genomes(w)
        _MODEL[(k, w, canon)] = (gs, [MR.rewrite(g, k, w, canon) for g in gs])
    return _MODEL[(k, w, canon)]


def _expected_k1(oracle, rw, k, S, canon):
    regs = np.stack([oracle.sketch_buffer(b, k=k, canon=canon, S=S)[0] for b in rw])
    counts = np.stack([R.counts_for(*oracle.kmer_count_buffer(b, k, canon)[:2], regs[i]) for i, b in enumerate(rw)])
    return regs, counts


class DevArrays:
    """packed stream, registers and counts of one batch in device memory under a (windowed) plan, the outputs pre-set to a pattern"""

    def __init__(self, ctx, sp, m, w, fill=0xAB):
        self.ctx = ctx
        packed, rs, rl, go = sp.arrays()
        self.n, self.m = go.size - 1, m
        self.plan = ctx.oph_plan(rs, rl, go, sp.k, w=w)
        self.packed = ctx.malloc(max(packed.size, 4))
        ctx.h2d(self.packed, packed)
        self.regs, self.counts = ctx.malloc(self.n * m * 8), ctx.malloc(self.n * m * 4)
        ctx.h2d(self.regs, np.full(self.n * m * 8, fill, np.uint8))
        ctx.h2d(self.counts, np.full(self.n * m * 4, fill, np.uint8))

    def read(self):
        regs, counts = np.empty((self.n, self.m), np.uint64), np.empty((self.n, self.m), np.uint32)
        self.ctx.sync()
        self.ctx.d2h(regs, self.regs)
        self.ctx.d2h(counts, self.counts)
        return regs, counts

    def close(self):
        for p in (self.packed, self.regs, self.counts):
            self.ctx.free(p)
        self.plan.close()


@pytest.mark.parametrize("k,w,S,canon", [(21, 30, 64, True), (31, 50, 100, True), (32, 100, 20000, False), (21, 37, 1024, False)])
def test_k1_and_k1b(d2g, gpu_ctx, oracle, k, w, S, canon):
    """S = 100: not a power of two; S = 20 000: the kernels' variant without registers in LDS.  Sketcher, plan + _dev and the
    K0-ingested stream give the oracle's registers and counts of the rewritten input"""
    gs, rw = _model(k, w, canon)
    eregs, ecounts = _expected_k1(oracle, rw, k, S, canon)
    assert (eregs[3] == R.M64).all() and (eregs[4] == R.M64).all() and (eregs[0] != R.M64).any()
    plain = oracle.sketch_buffer(gs[0], k=k, canon=canon, S=S)[0]
    assert not np.array_equal(plain, eregs[0])                         # the window changes what is sketched
    sp = _pack(d2g, gs, k)
    sk = gpu_ctx.sketcher()
    sk.set_window(w)
    regs, counts = sk.run_counts(sp, S, canon=canon)
    assert np.array_equal(regs, eregs) and np.array_equal(counts, ecounts)
    assert np.array_equal(sk.run(sp, S, canon=canon), eregs)
    # the plan + _dev forms
    dv = DevArrays(gpu_ctx, sp, d2g.oph_m(S), w)
    assert dv.plan.nkmers == sum(b.count(b">") for b in rw)          # emissions, not k-mers
    gpu_ctx.oph_sketch_dev(dv.plan, dv.packed, S, dv.regs, canon=canon)
    gpu_ctx.oph_count_dev(dv.plan, dv.packed, S, dv.regs, dv.counts, canon=canon)
    dregs, dcounts = dv.read()
    assert np.array_equal(dregs, eregs) and np.array_equal(dcounts, ecounts)
    dv.close()
    # the device FASTA parser's stream (packed == NULL)
    runs = sk.ingest_fasta(gs, k)
    assert np.array_equal(sk.run_ingested(runs, S, canon=canon), eregs)
    # w <= k switches the window off: the plain oracle
    for off in (0, k, k - 1):
        sk.set_window(off)
        assert np.array_equal(sk.run(sp, S, canon=canon)[0], plain)
    dv = DevArrays(gpu_ctx, sp, d2g.oph_m(S), k)
    gpu_ctx.oph_sketch_dev(dv.plan, dv.packed, S, dv.regs, canon=canon)
    assert np.array_equal(dv.read()[0][0], plain) and dv.plan.nkmers == sum(sp.nkmers(g) for g in range(len(gs)))
    dv.close()
    sk.close()


@pytest.mark.parametrize("k,w,canon", [(21, 30, True), (32, 40, False)])
def test_mincount_bmh_distinct_and_sets(d2g, gpu_ctx, oracle, k, w, canon, monkeypatch):
    S = 64
    gs, rw = _model(k, w, canon)
    kc = [oracle.kmer_count_buffer(b, k, canon)[:2] for b in rw]
    assert max(int(c.max()) for _, c in kc if c.size) >= 3             # consecutive windows share their minimizer: counts well above 1
    sp = _pack(d2g, gs, k)
    sk = gpu_ctx.sketcher()
    sk.set_window(w)
    # -m 2: registers over the k-mers emitted at least twice, and K1b's counts of them
    regs, counts = sk.run_mincount(sp, S, 2, canon=canon, counts=True)
    for g, (keys, cnts) in enumerate(kc):
        er, ec = Q.closed_form(keys, cnts, d2g.oph_m(S), 2)
        assert np.array_equal(regs[g], er) and np.array_equal(counts[g], ec), g
    # --multiset: BagMinHash over (k-mer, window positions), with and without a count threshold
    for thr in (0.0, 1.0):
        sig, tw = sk.run_bmh(sp, S, canon=canon, count_threshold=thr)
        for g, b in enumerate(rw):
            e = oracle.bmh_sketch_buffer(b, k, S, canon, count_threshold=thr)
            assert tw[g] == e[1] and np.array_equal(sig[g].view(np.uint64), e[0].view(np.uint64)), (thr, g)
    assert tw[3] == 0 and tw[4] == 0
    # --parse-by-seq's distinct count
    assert sk.run_distinct(sp, canon=canon).tolist() == [keys.size for keys, _ in kc]
    # --set / --countdict
    keys, counts, off, cards = sk.run_sets(sp, canon=canon)
    for g, (ek, ec) in enumerate(kc):
        assert np.array_equal(keys[int(off[g]):int(off[g + 1])], ek) and np.array_equal(counts[int(off[g]):int(off[g + 1])], ec)
    # the plan + _dev forms against the sketcher's
    dv = DevArrays(gpu_ctx, sp, d2g.oph_m(S), w)
    gpu_ctx.oph_sketch_mincount_dev(dv.plan, dv.packed, S, 2, dv.regs, canon=canon)
    assert np.array_equal(dv.read()[0], regs)
    tw_dev = gpu_ctx.malloc(dv.n * 8)
    gpu_ctx.bmh_sketch_dev(dv.plan, dv.packed, S, dv.regs, tw_dev, canon=canon, count_threshold=1.0)
    dsig, dtw = np.empty((dv.n, S), np.float64), np.empty(dv.n, np.float64)
    gpu_ctx.sync()
    gpu_ctx.d2h(dsig, dv.regs)
    gpu_ctx.d2h(dtw, tw_dev)
    assert np.array_equal(dsig.view(np.uint64), sig.view(np.uint64)) and np.array_equal(dtw, tw)
    gpu_ctx.free(tw_dev)
    dv.close()
    # the compact K3 walkers (k3c_hist / k3c_scatter) and the two-level split walk the same minimizers
    if k <= 21:
        monkeypatch.setenv("D2G_K3_COMPACT", "1")
        sig2, tw2 = sk.run_bmh(sp, S, canon=canon, count_threshold=1.0)
        assert np.array_equal(sig2.view(np.uint64), sig.view(np.uint64)) and np.array_equal(tw2, tw)
        monkeypatch.delenv("D2G_K3_COMPACT")
    sk.close()


@pytest.mark.parametrize("k,w,canon", [(21, 30, True), (5, 7, False)])
def test_windowed_filter(d2g, gpu_ctx, oracle, k, w, canon):
    """the filter file is enumerated with the same window: only ITS minimizers are in the set, and the input's minimizers meet it"""
    S = 64
    gs, _ = _model(k, w, canon)
    g0 = gs[0].split(b"\n")[1]
    filt = [_fa(g0[1000:6000], "slice"), _fa(_seq(505, 1000), "other")]
    fem = [v for f in filt for v in MR.fasta_emissions(f, k, w, canon, fast=True)]
    fset = set(fem)
    rw = [MR.rewrite(g, k, w, canon, keep=lambda v: v not in fset) for g in gs]
    f = gpu_ctx.kmer_filter(_pack(d2g, filt, k), canon, w=w)
    assert f.info()[:2] == (len(fem), len(fset))                       # occurrences = the filter's emissions
    asked = np.array(sorted(fset)[:50] + [v ^ 1 for v in sorted(fset)[:50]], np.uint64)
    assert f.contains(asked).tolist() == [int(v) in fset for v in asked]
    sp = _pack(d2g, gs, k)
    sk = gpu_ctx.sketcher()
    sk.set_window(w)
    sk.set_filter(f)
    eregs, ecounts = _expected_k1(oracle, rw, k, S, canon)
    regs, counts = sk.run_counts(sp, S, canon=canon)
    assert np.array_equal(regs, eregs) and np.array_equal(counts, ecounts)
    assert rw[0].count(b">") < MR.rewrite(gs[0], k, w, canon).count(b">")          # something was filtered
    sig, tw = sk.run_bmh(sp, S, canon=canon)
    for g, b in enumerate(rw):
        e = oracle.bmh_sketch_buffer(b, k, S, canon)
        assert tw[g] == e[1] and np.array_equal(sig[g].view(np.uint64), e[0].view(np.uint64)), g
    # the device-resident build over a windowed plan gives the same table
    dv = DevArrays(gpu_ctx, _pack(d2g, [b"".join(filt)], k), 1, w)
    f2 = gpu_ctx.kmer_filter_dev(dv.plan, dv.packed, canon)
    assert f2.info()[:2] == (len(fem), len(fset)) and f2.contains(asked).tolist() == f.contains(asked).tolist()
    dv.close()
    # a filter of another window does not fit: D2G_ERR_INVALID before anything is written
    for other in (0, w + 1):
        sk.set_window(other)
        for call in (lambda: sk.run(sp, S, canon=canon), lambda: sk.run_bmh(sp, S, canon=canon), lambda: sk.run_distinct(sp, canon=canon)):
            with pytest.raises(d2g.D2GError) as e:
                call()
            assert e.value.status == INVALID and "another window" in str(e.value)
    dv = DevArrays(gpu_ctx, sp, d2g.oph_m(S), 0)
    dv.plan.set_filter(f)
    with pytest.raises(d2g.D2GError) as e:
        gpu_ctx.oph_sketch_dev(dv.plan, dv.packed, S, dv.regs, canon=canon)
    assert e.value.status == INVALID and "another window" in str(e.value) and (dv.read()[0] == 0xABABABABABABABAB).all()
    dv.close()
    sk.close()
    f2.close()
    f.close()


@pytest.mark.parametrize("k,w,canon", [(21, 30, True), (32, 33, False)])
def test_screen(d2g, gpu_ctx, oracle, k, w, canon):
    """`contain` over a windowed database: the screen counts window positions per database key"""
    S = 64
    gs, rw = _model(k, w, canon)
    sp = _pack(d2g, gs, k)
    sk = gpu_ctx.sketcher()
    sk.set_window(w)
    db = d2g.oph_kmer_ids(sk.run(sp, S, canon=canon)[:3], S)           # the k-mers behind the registers of three windowed sketches
    sc = gpu_ctx.screen(db, k, canon=canon, nrows=len(gs))
    sk.run_screen(sp, sc, list(range(len(gs))), canon=canon)
    m, s = sc.result()
    for g, b in enumerate(rw):
        keys, cnts, nk = oracle.kmer_count_buffer(b, k, canon)
        em, es = CR.closed_form(db, keys, cnts)
        assert np.array_equal(m[g], em) and np.array_equal(s[g], es), g
        assert sc.fed(g) == nk                                         # fed = window positions
    assert m[0][0] > 0 and m[3].sum() == 0 and m[4].sum() == 0
    # the plan form adds the same counts once more
    dv = DevArrays(gpu_ctx, sp, 1, w)
    sc.add_dev(dv.plan, dv.packed, list(range(len(gs))))
    m2, s2 = sc.result()
    assert np.array_equal(m2, m) and np.array_equal(s2, 2 * s)
    dv.close()
    # without the window the same screen sees every k-mer: more hits for the genome itself
    sc.reset()
    sk.set_window(0)
    sk.run_screen(sp, sc, list(range(len(gs))), canon=canon)
    m3, s3 = sc.result()
    keys, cnts, nk = oracle.kmer_count_buffer(gs[0], k, canon)
    em, es = CR.closed_form(db, keys, cnts)
    assert np.array_equal(m3[0], em) and np.array_equal(s3[0], es) and sc.fed(0) == nk == 70000 - k + 1
    sc.close()
    sk.close()


def test_window_above_the_cap_is_unsupported(d2g, gpu_ctx):
    k = 21
    sp = _pack(d2g, [_fa(_seq(1, 9000))], k)
    sk = gpu_ctx.sketcher()
    sk.set_window(k + 4096)                                            # q = 4097
    with pytest.raises(d2g.D2GError) as e:
        sk.run(sp, 64)
    assert e.value.status == UNSUPPORTED and "window" in str(e.value)
    packed, rs, rl, go = sp.arrays()
    with pytest.raises(d2g.D2GError) as e:
        gpu_ctx.oph_plan(rs, rl, go, k, w=k + 4096)
    assert e.value.status == UNSUPPORTED
    # the cap itself works: q = 4096
    sk.set_window(k + 4095)
    _check_sets(d2g, sk, [_fa(_seq(1, 9000))], k, k + 4095, True)
    sk.close()
